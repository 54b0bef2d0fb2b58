"""Host side of the HIP UNet forward: weight repacking, buffer planning and the launch sequence.

The reference runs ``UNetModel.forward`` (``unet.py:1499-1836``) / ``UNetModelPhosc.forward``
(``unetPhosc.py:1068-1159``) as ~150 ATen kernels over NCHW fp32 tensors.  Here the same arithmetic is a static
list of launches of the kernels in ``csrc/`` over token-major (NHWC) buffers:

  * every convolution / linear is ``wd_gemm`` (tap-gather GEMM on MFMA, split-bf16 operands);
  * GroupNorm(+SiLU) is ``wd_gn_stats`` + ``wd_gn_apply`` which writes the GEMM operand planes directly - the
    channel concat of the decoder (``torch.cat([h, hs.pop()], 1)``, unet.py:1750) is never materialised, the two
    halves are normalised into one plane buffer; the 1x1 skip projection of a ResBlock is a second K-segment of
    its last 3x3 GEMM; nearest-x2 upsampling / stride-2 are gather tables of the same GEMM;
  * step-invariant work (CharacterEncoder, K/V projections of every cross-attention) lives in ``cond`` ops that
    ``Diffusion.sampling`` runs once per call, the per-step ops are captured into one hipGraph.

Torch is used for device memory, the weight repack at load time and stream handles only.
"""
from __future__ import annotations

import collections
import ctypes as C
import math
import os
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _native as N
from .layers import (DownsampleParams, ResBlockParams, SpatialTransformerParams, UpsampleParams)


# ----------------------------------------------------------------------------------------------------------
def conv_gather_table(h: int, w: int, mode: str) -> Tuple[np.ndarray, int, int]:
    """int32 [9][h_out*w_out] source position (or -1 = zero padding) per 3x3 tap.

    mode 'same': 3x3 pad 1 (unet.py:595); 'down': 3x3 stride 2 pad 1 (unet.py:540-542);
    'up': nearest x2 then 3x3 pad 1 (unet.py:497-499); 'down_rb': zero padding on the right and bottom only, then 3x3 stride 2
    pad 0 (the ``Downsample2D`` of the AutoencoderKL encoder: output (y, x) reads (2y + ky, 2x + kx)) - (h, w) is the INPUT size
    in all modes."""
    if mode == "same":
        ho, wo = h, w
    elif mode == "down":
        ho, wo = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
    elif mode == "up":
        ho, wo = 2 * h, 2 * w
    elif mode == "down_rb":
        ho, wo = (h - 2) // 2 + 1, (w - 2) // 2 + 1
    else:
        raise ValueError(mode)
    yy, xx = np.meshgrid(np.arange(ho), np.arange(wo), indexing="ij")
    tab = np.full((9, ho * wo), -1, dtype=np.int32)
    for tap in range(9):
        dy, dx = tap // 3 - 1, tap % 3 - 1
        if mode == "same":
            sy, sx = yy + dy, xx + dx
            ok = (sy >= 0) & (sy < h) & (sx >= 0) & (sx < w)
        elif mode == "down":
            sy, sx = 2 * yy + dy, 2 * xx + dx
            ok = (sy >= 0) & (sy < h) & (sx >= 0) & (sx < w)
        elif mode == "down_rb":
            sy, sx = 2 * yy + dy + 1, 2 * xx + dx + 1
            ok = (sy < h) & (sx < w)
        else:
            uy, ux = yy + dy, xx + dx  # coordinates in the upsampled map
            ok = (uy >= 0) & (uy < ho) & (ux >= 0) & (ux < wo)
            sy, sx = uy // 2, ux // 2
        idx = sy * w + sx
        tab[tap] = np.where(ok, idx, -1).reshape(-1)
    return tab, ho, wo


def upsample_phase_tables(h: int, w: int) -> Tuple[np.ndarray, np.ndarray]:
    """Nearest x2 upsample + 3x3 / pad 1 convolution (Upsample.forward, unet.py:488-499) as four 2x2 convolutions of the SOURCE map,
    one per output phase (py, px) = (row parity, column parity): the taps of the 3x3 kernel that fall on the same source pixel are
    summed (``upsample_phase_weights``), 4 taps instead of 9.  Output rows of a sample are phase-major: q = (2 py + px) * h*w + y*w + x
    is output pixel (2y + py, 2x + px).

    Returns (int32 [4 taps][4*h*w] source position or -1, tap = 2 dy + dx reads source (y + dy - 1 + py, x + dx - 1 + px);
             int32 [4*h*w]: the row q that holds raster position (Y, X) of the 2h x 2w map)."""
    hw = h * w
    tab = np.full((4, 4 * hw), -1, dtype=np.int32)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    for py in range(2):
        for px in range(2):
            ph = 2 * py + px
            for dy in range(2):
                for dx in range(2):
                    sy, sx = yy + dy - 1 + py, xx + dx - 1 + px
                    ok = (sy >= 0) & (sy < h) & (sx >= 0) & (sx < w)
                    tab[2 * dy + dx, ph * hw:(ph + 1) * hw] = np.where(ok, sy * w + sx, -1).reshape(-1)
    Y, X = np.meshgrid(np.arange(2 * h), np.arange(2 * w), indexing="ij")
    perm = ((2 * (Y % 2) + (X % 2)) * hw + (Y // 2) * w + (X // 2)).reshape(-1).astype(np.int32)
    return tab, perm


def upsample_phase_weights(w: torch.Tensor) -> torch.Tensor:
    """[N, C, 3, 3] -> [4 phases][4 taps][N][C] fp32: kernel rows {0} / {1, 2} feed source rows y - 1 / y of an even output row,
    {0, 1} / {2} feed y / y + 1 of an odd one (the same for columns); phase = 2 py + px, tap = 2 dy + dx."""
    sel = torch.tensor([[[1., 0., 0.], [0., 1., 1.]], [[1., 1., 0.], [0., 0., 1.]]], dtype=torch.float32, device=w.device)  # [parity][d][k]
    out = torch.einsum("pdk,qel,nckl->pqdenc", sel, sel, w.detach().float())
    n, c = w.shape[0], w.shape[1]
    return out.reshape(4, 4, n, c).contiguous()


def geglu_interleave(w: torch.Tensor, g: int = 32) -> torch.Tensor:
    """Rows [x | gate] (unet.py:128 ``chunk(2)``) -> blocks of ``g`` x-rows followed by their ``g`` gate rows, so
    that one BN = 2g column tile of ``wd_gemm`` holds both halves of ``g`` output columns."""
    inner = w.shape[0] // 2
    assert inner % g == 0
    x = w[:inner].reshape(inner // g, g, *w.shape[1:])
    gt = w[inner:].reshape(inner // g, g, *w.shape[1:])
    return torch.stack([x, gt], dim=1).reshape(w.shape)


def wdirect_fills_chip(m: int, n: int) -> bool:
    """Policy: the 64 x 320 weights-to-registers kernel (wd_gemm_args.w_layout 3) is taken where its tiles alone fill the chip."""
    return ((m + 63) // 64) * (n // 320) >= 256


def geglu_tile(inner: int) -> int:
    """GEMM tile for a GEGLU projection with ``inner`` output columns: 128x160 when 80 divides it."""
    return 128160 if inner % 80 == 0 else 128064


def slab_order(wp: torch.Tensor, ntaps0: int, c0: int, c1: int = 0) -> torch.Tensor:
    """[..., N, ktot] (k = tap-major/channel-minor of src0, then src1) -> "slab order" [..., stages, N, 32]:
    stage = (32-channel chunk of src0, tap) chunk-major, then the 32-channel chunks of src1 (wd_gemm w_layout 1)."""
    lead = wp.shape[:-2]
    n = wp.shape[-2]
    k0 = ntaps0 * c0
    w0 = wp[..., :k0].reshape(*lead, n, ntaps0, c0 // 32, 32)
    nl = len(lead)
    w0 = w0.permute(*range(nl), nl + 2, nl + 1, nl, nl + 3).reshape(*lead, (c0 // 32) * ntaps0, n, 32)
    if c1:
        w1 = wp[..., k0:].reshape(*lead, n, c1 // 32, 32).permute(*range(nl), nl + 1, nl, nl + 2)
        w0 = torch.cat([w0, w1], dim=nl)
    return w0.contiguous()


def slab_span(tab: Optional[np.ndarray], hw_out: int, hw_src: int, m: int, bm: int = 128) -> int:
    """Largest (max - min + 1) of the gathered source rows over the bm-row output panels (wd_gemm slab_rows)."""
    if tab is None:
        return bm
    period = int(np.lcm(bm, hw_out))
    mt = min(m, 2 * period)
    rows = np.arange(mt)
    b, p = rows // hw_out, rows % hw_out
    src = np.where(tab[:, p] >= 0, b[None, :] * hw_src + tab[:, p], -1)  # [ntaps, mt]
    span = 0
    for r0 in range(0, mt, bm):
        blk = src[:, r0:r0 + bm]
        valid = blk[blk >= 0]
        if valid.size:
            span = max(span, int(valid.max() - valid.min() + 1))
    return span


_PARAM_GEN = [0]  # bumped whenever any nn.Module registers a Parameter (see UNetEngine._signature)
_NATIVE_WRITES = [0]  # bumped whenever a kernel of this package rewrites parameters in place (optimiser step, EMA)


def note_native_write():
    """``wd_adamw_multi`` / ``wd_ema_update`` change parameter storage behind autograd's back (no ``Tensor._version`` bump): every
    engine re-derives its packed operands before its next use.  (A public counter of our own instead of the private
    ``torch._C._autograd._unsafe_set_version_counter``.)"""
    _NATIVE_WRITES[0] += 1

PLAN_CACHE_SIZE = int(os.environ.get("WDIFF_PLAN_CACHE", "4"))  # launch plans kept per engine (least recently used evicted)


def _bump_param_gen(*_a):
    _PARAM_GEN[0] += 1


torch.nn.modules.module.register_module_parameter_registration_hook(_bump_param_gen)

FILM_CHUNK_ROWS = int(os.environ.get("WDIFF_FILM_CHUNK_ROWS", "8192"))  # rows (timesteps x batch) of the resident FiLM chunk


class _Recipe:
    __slots__ = ("name", "planes", "rows", "cols", "shape", "pieces")

    def __init__(self, name, planes, rows=0, cols=0, shape=None):
        self.name, self.planes, self.rows, self.cols, self.shape, self.pieces = name, planes, rows, cols, shape, []

    @staticmethod
    def _nct(w):
        return w.shape[0], w.shape[1], (w.shape[2] * w.shape[3] if w.dim() == 4 else 1)

    def fwd(self, w, row_off=0, col_off=0, g=0):
        """[N, C(, kh, kw)] parameter -> rows row_off.., columns col_off + tap*C + c of this matrix."""
        n, c, t = self._nct(w)
        assert row_off + n <= self.rows and col_off + t * c <= self.cols, self.name
        self.pieces.append((0, w, None, n, c, t, row_off, col_off, 0, g))
        return self

    def bwd(self, w, col_off=0, npad=None):
        """[N, C(, kh, kw)] parameter -> rows c, columns col_off + tap*npad + n (the data-gradient operand)."""
        n, c, t = self._nct(w)
        npad = n if npad is None else npad
        assert c <= self.rows and col_off + t * npad <= self.cols, self.name
        self.pieces.append((1, w, None, n, c, t, 0, col_off, npad, 0))
        return self

    def vec(self, p, p2=None, off=0, g=0):
        self.pieces.append((2, p, p2, p.numel(), 1, 1, 0, off, 0, g))
        return self

    def host(self) -> torch.Tensor:
        """The packed operand in fp32, computed with torch on the parameters' device: the specification of
        ``wd_repack_multi``'s index mapping (used by the tests; the product path never calls it)."""
        first = self.pieces[0][1]
        out = torch.zeros((self.rows, self.cols) if self.planes else (int(torch.tensor(self.shape).prod()),),
                          dtype=torch.float32, device=first.device)
        for (mode, p, p2, n, c, t, row_off, col_off, npad, g) in self.pieces:
            src = p.detach().float()
            if mode == 2:
                v = src.reshape(-1) + (p2.detach().float().reshape(-1) if p2 is not None else 0)
                out[col_off:col_off + n] = geglu_interleave(v, g) if g else v
                continue
            w3 = src.reshape(n, c, t)
            if mode == 0:
                blk = w3.permute(0, 2, 1).reshape(n, t * c)
                out[row_off:row_off + n, col_off:col_off + t * c] = geglu_interleave(blk, g) if g else blk
            else:
                blk = torch.zeros(c, t, npad, dtype=torch.float32, device=first.device)
                blk[:, :, :n] = w3.permute(1, 2, 0)
                out[:c, col_off:col_off + t * npad] = blk.reshape(c, t * npad)
        return out if self.planes else out.reshape(self.shape)


class RecipeBook(dict):
    """name -> _Recipe.  Matrices become split-bf16 planes [2, rows, cols]; vectors stay fp32."""

    def matrix(self, name, rows, cols) -> _Recipe:
        self[name] = _Recipe(name, True, rows, cols)
        return self[name]

    def vector(self, name, p, p2=None, g=0) -> _Recipe:
        self[name] = _Recipe(name, False, shape=tuple(p.shape)).vec(p, p2, 0, g)
        return self[name]

    def vector_cat(self, name, ps) -> _Recipe:
        r = _Recipe(name, False, shape=(sum(p.numel() for p in ps),))
        off = 0
        for p in ps:
            r.vec(p, None, off)
            off += p.numel()
        self[name] = r
        return r

    def linear(self, name, lin):
        self.matrix(name + ".w", lin.weight.shape[0], lin.weight.shape[1]).fwd(lin.weight)
        if lin.bias is not None:
            self.vector(name + ".b", lin.bias)

    @staticmethod
    def frag_ok(r) -> bool:
        """Can ``wd_repack_multi`` write this matrix fragment-major itself (mode 3)?"""
        return r.planes and r.rows % 16 == 0 and r.cols % 32 == 0 and all(
            mode == 0 and c % 32 == 0 and t in (1, 9) and col_off % 2 == 0 and row_off >= 0
            for (mode, p, p2, n, c, t, row_off, col_off, npad, g) in r.pieces)

    def device_table(self, lib, dst: Dict[str, torch.Tensor], dev, frag: Optional[Dict[str, torch.Tensor]] = None):
        """Serialises the pieces into the entry table of ``wd_repack_multi`` (include/wdiff_hip.h).  ``frag``: name -> the
        fragment-major image to write as well (mode 3) for the matrices ``frag_ok`` accepts."""
        tile, vchunk = lib.wd_repack_tile(), lib.wd_repack_vchunk()
        recs, c0 = [], 0
        for name, r in self.items():
            d = dst[name]
            for (mode, p, p2, n, c, t, row_off, col_off, npad, g) in r.pieces:
                assert p.is_cuda and p.dtype == torch.float32 and p.is_contiguous(), name
                if mode == 2:
                    hi, lo, ld, ntc = d.data_ptr() + 4 * col_off, 0, 0, 1
                    nch = (n + vchunk - 1) // vchunk
                else:
                    ld = r.cols
                    o = 2 * (row_off * ld + col_off)
                    hi, lo = d[0].data_ptr() + o, d[1].data_ptr() + o
                    ntc = (c + tile - 1) // tile
                    nch = (((npad if mode == 1 else n) + tile - 1) // tile) * ntc
                recs.append(N.WdRepackEntry(p.data_ptr(), p2.data_ptr() if p2 is not None else 0, hi, lo, n, c, t,
                                            mode, npad, ld, g, ntc, c0, 0, 0))
                c0 += nch
                if frag is not None and name in frag and self.frag_ok(r):
                    f = frag[name]
                    recs.append(N.WdRepackEntry(p.data_ptr(), 0, f[0].data_ptr(), f[1].data_ptr(), n, c, t, 3, 0,
                                                r.rows, g, ntc, c0, row_off, col_off))
                    c0 += nch
        raw = torch.frombuffer((N.WdRepackEntry * len(recs))(*recs), dtype=torch.uint8).to(dev)
        return raw, c0, len(recs)


class Act:
    """A token-major fp32 feature map [B*h*w, c] on the device."""
    __slots__ = ("t", "c", "h", "w", "stats", "prod", "perm")

    def __init__(self, t, c, h, w, stats=None, prod=None, perm=None):
        self.t, self.c, self.h, self.w = t, c, h, w
        self.perm = perm    # None, or int32 [h*w] on the device: the row (inside its sample) that holds raster position p - the
        #                     phase-major output of an Upsample (only the two-source GroupNorm of a decoder block reads such a map)
        self.stats = stats  # (part tensor [B, nchunk, c / part_cpg, 2] f64, nchunk, part_cpg) once known
        self.prod = prod    # the WdGemmArgs of the GEMM whose epilogue writes ``t``: a consumer that wants the operand planes of
        #                     this very tensor asks that epilogue for them instead of launching wd_split


# How one SpatialTransformer is launched (UNetEngine._st_form) and what every stage of it needs to know:
#   form   "one-launch" (GroupNorm to proj_out in one launch), else how the chain runs attn1 / attn2: "pair" | "folded" | "phosc" | "plain"
#   tail   how the last block's feed-forward meets proj_out: "ff+proj" | "two-source" | "proj_out"
#   M = B * hw token rows of inner = heads * d channels (the map has c), L context keys
#   tap    an attention-map tap of the plan: one wd_xattn_maps launch behind the attentions
#   gn_in  proj_in applies the GroupNorm itself while it stages the fp32 map (no wd_gn_apply launch)
#   xfold  the cross-attentions run folded (wd_xattn_fold): one launch each, or one for the pair
StForm = collections.namedtuple("StForm", "form tail B h w c hw M heads d inner L tap gn_in xfold")


def gather_hint(mode: str, w: int, wo: int) -> Tuple[int, int]:
    """(same_w, down_w) of the table ``conv_gather_table(h, w, mode)`` with output width ``wo``: the image width the GEMM planner
    may pass as wd_gemm_args.slab_rows, with which the kernel COMPUTES the source rows of the pad-1 geometry instead of reading the
    table.  'same' (3x3 / pad 1 / stride 1): the image width; 'down' (stride 2): the OUTPUT width.  Every other table must be read,
    so it gets no hint - 'down_rb' in particular pads right and bottom only."""
    return (w if mode == "same" else 0), (wo if mode == "down" else 0)


class GatherTable(NamedTuple):
    """A tap-gather table (wd_src.gather) with what the planners know about it."""
    dev: torch.Tensor   # int32 [ntaps][ho * wo] on the device
    ho: int
    wo: int
    host: np.ndarray    # the same table on the host (slab_span)
    same_w: int = 0     # gather_hint; a table not made by conv_gather_table has none
    down_w: int = 0


class Src(NamedTuple):
    """One A-operand source of a GEMM being planned: the wd_src the kernel reads and the record of its gather table."""
    raw: N.WdSrc
    tab: Optional[GatherTable] = None


class GemmOp(NamedTuple):
    """A planned wd_gemm / wd_ff_fused launch: its args (kept alive by the plan, still open to the fusions of a consumer:
    ``Act.prod``) and what its epilogue makes beside the output."""
    args: object                           # N.WdGemmArgs | N.WdFfArgs
    stats: Optional[tuple] = None          # ``Act.stats`` of the output, where the launch sums the GroupNorm statistics
    ln_pl: Optional[torch.Tensor] = None   # planes of the LayerNorm of the output, where the launch writes them


# The kernel form UNetEngine._gemm_form picks for one GEMM: kind "slab-order" | "wdirect" | "whole-k" | "generic", and the
# wd_gemm_args fields that select it (w_layout, tile, slab_rows).
GemmForm = collections.namedtuple("GemmForm", "kind fields")


class Plan:
    def __init__(self):
        self.cond: List[tuple] = []
        self.step: List[tuple] = []
        self.keep: List[object] = []
        self.out: Optional[torch.Tensor] = None
        # the zeroed arrival counters the plan's split-K launches take their ranges from (UNetEngine._give_tickets)
        self.tickets: Optional[torch.Tensor] = None
        self.ticket_off = 0
        # attention maps (UNetEngine.plan attn_maps): the tapped SpatialTransformers, their buffers fp32 [B, h*w, L] and (h, w),
        # the accumulate form's weight table
        self.map_taps: tuple = ()
        self.maps: List[torch.Tensor] = []
        self.map_hw: List[tuple] = []
        self.map_w: Optional[torch.Tensor] = None

    @staticmethod
    def _run(ops, stream):
        for fn, args, what in ops:
            rc = fn(*args, stream)
            if rc != 0:
                N.check(rc, what)

    def run_cond(self, stream):
        self._run(self.cond, stream)

    def run_film(self, stream):
        """Per-call part of the tabulated FiLM path: the time MLP of every timestep.  The chunk of the table a step reads is
        brought in by ``film_prepare(t, stream)`` (a no-op closure when the plan has no table)."""
        self._run(getattr(self, "film", []), stream)
        self.film_loaded = -1  # writer ids / weights may have changed since the last call: no chunk is valid

    @staticmethod
    def film_prepare(t, stream):
        return False

    def run_step(self, stream):
        self._run(self.step, stream)

    def run_step1(self, stream):
        """The second forward of a step of the two-forward interpolation plan (``UNetEngine.plan`` mix = 2)."""
        self._run(self.step1, stream)


def check_writer_keep(writer_keep, B: int) -> torch.Tensor:
    """The ``writer_keep`` argument as a uint8 tensor [B] (1: the sample keeps its writer term); raises for anything else."""
    k = torch.as_tensor(writer_keep)
    if k.dtype not in (torch.bool, torch.uint8) or tuple(k.shape) != (B,):
        raise ValueError(f"writer_keep must be a bool / uint8 tensor [{B}], False or None, got {k.dtype} {tuple(k.shape)}")
    return (k != 0).to(torch.uint8)


def _ptr(t: Optional[torch.Tensor], byte_off: int = 0):
    return None if t is None else t.data_ptr() + byte_off


class UNetEngine:
    """Builds and runs the launch plan for one model instance."""

    fold_proj = False   # (class default: _recipes() of an engine that never ran __init__ describes the parameters' own operands only)

    def __init__(self, model, variant: str):
        self.model = model
        self.variant = variant  # 'base' | 'phosc'
        self.lib = N.lib()
        self.npass = 3
        self._sig = None
        self._ps, self._ps_gen = None, -1
        self._pack = None
        self._w: Dict[str, torch.Tensor] = {}
        self._w3: Dict[str, torch.Tensor] = {}      # slab-order copies of the matrices the v3 kernel consumes
        self._w3_meta: Dict[str, tuple] = {}
        self._wf: Dict[str, torch.Tensor] = {}      # fragment-major copies of the matrices the weights-to-registers kernel reads
        # 64 x 320 tiles with the weights loaded straight into the MFMA operand registers (csrc/wd_gemmw.hip): the 320-column
        # layers whose grid fills the chip without a K cut
        self.use_wdirect = os.environ.get("WDIFF_GEMM_WDIRECT", "1") != "0"
        # ... with the rows of a 3x3 / pad 1 / stride 1 source copied into an LDS slab once per 64-channel chunk instead of gathered per
        # tap (wd_gemmw_kernel<..., SLAB>).  wd_gemm decides where that form is legal and reads the same variable for its default; an
        # engine built while it is set passes its value with every launch (wd_gemm_args.dbg WD_GEMMW_SLAB_ON / _OFF).
        self.gemmw_slab = {None: None, "0": False}.get(os.environ.get("WDIFF_GEMMW_SLAB"), True)
        # the batched epilogue of the 64-row tiles (wd_epilogue_rows: 64 x 320, 64 x 80, wd_ff_fused).  wd_gemm / wd_ff_fused decide where
        # that form is legal and read the same variable for their default; an engine built while it is set passes its value with every
        # such launch (wd_gemm_args.dbg / wd_ff_args.dbg WD_EPI_BATCH_ON / _OFF).
        self.epi_batch = {None: None, "0": False}.get(os.environ.get("WDIFF_EPI_BATCH"), True)
        # Upsample as four 2x2 convolutions of the source map (one per output phase, 4 taps instead of 9; upsample_phase_tables)
        self.use_up_phases = os.environ.get("WDIFF_UPSAMPLE_PHASES", "1") != "0"
        self._derived: Dict[str, tuple] = {}   # name -> (persistent fp32 tensor, function that recomputes it from the parameters)
        self.use_smallmap = os.environ.get("WDIFF_GEMM_SMALLMAP", "1") != "0"  # 64 x 80 whole-K tiles for 3x3 layers over 64-position samples
        # GEGLU feed-forward + residual in one launch per 64-token panel, hidden activations on chip (csrc/wd_ff.hip)
        self.fuse_ff = os.environ.get("WDIFF_FUSE_FF", "1") != "0"
        self.fuse_proj = os.environ.get("WDIFF_FUSE_PROJ", "1") != "0"   # ... and proj_out + residual in the same launch
        # GroupNorm (+ SiLU) of a convolution's input applied while the weights-to-registers kernel stages its rows (no wd_gn_apply
        # launch, no operand planes of the normalised map)
        self.fuse_ln = os.environ.get("WDIFF_FUSE_LN", "1") != "0"  # LayerNorm of a 320-column GEMM result in its own epilogue
        self.fuse_gn_in = int(os.environ.get("WDIFF_FUSE_GN_IN", "1"))  # 0 off, 1 the 1x1 consumers, 2 the 3x3 consumers too
        self.use_slab = os.environ.get("WDIFF_SLAB", "0") != "0"
        self.fuse_stats = os.environ.get("WDIFF_FUSE_STATS", "1") != "0"
        self.fuse_xattn = os.environ.get("WDIFF_FUSE_XATTN", "1") != "0"
        # row-shared-taps convolution kernel (29 % fewer DMA pieces, but measured 15 % slower than the generic kernel so far)
        self.use_conv3 = os.environ.get("WDIFF_CONV3", "0") != "0"
        if (self.use_slab or self.use_conv3) and not self.lib.wd_gemm_experimental():
            raise N.NativeError("WDIFF_SLAB / WDIFF_CONV3 need a library built with WDIFF_EXPERIMENTAL=1 "
                                "(python -m worddiffusion_amd.build --force)")
        self.fuse_xattn_pair = os.environ.get("WDIFF_FUSE_XATTN_PAIR", "1") != "0"
        # the whole base-model SpatialTransformer of the 8 x 32 level (GroupNorm + proj_in, both folded cross-attentions, the
        # feed-forward, proj_out) as one wd_ff_fused launch per 64-token panel; 0: the three-launch chain
        self.fuse_st = os.environ.get("WDIFF_FUSE_ST", "1") != "0"
        # proj_out folded into the feed-forward's second product (no non-linearity between them): W32 = W3 W2 and b32 = W3 b2 + b3
        # are derived once per weight refresh (wd_linear_fold), the materialised x' = ff2(...) + tok2 and its launch / passes go
        self.fold_proj = os.environ.get("WDIFF_FOLD_PROJ", "1") != "0"
        self.fuse_out = os.environ.get("WDIFF_FUSE_OUT", "1") != "0"
        self.fuse_in = os.environ.get("WDIFF_FUSE_IN", "1") != "0"         # the first convolution as one direct fp32 launch
        self.pack_kv = os.environ.get("WDIFF_PACK_KV", "1") != "0"         # long-context cross-attention: K/V images built once per call
        self.fuse_gn2 = os.environ.get("WDIFF_FUSE_GN2", "1") != "0"       # GroupNorm over [h | skip]: one apply launch for both
        self.fuse_gn = os.environ.get("WDIFF_FUSE_GN", "1") != "0"         # GroupNorm in the producer's split-K combine launch
        self.fuse_split = os.environ.get("WDIFF_FUSE_SPLIT", "1") != "0"   # resample inputs: planes from the producer's epilogue
        self._plans: Dict[tuple, Plan] = {}
        self._tabs: Dict[tuple, object] = {}   # (h, w, mode) -> GatherTable; (h, w, "up4") -> (GatherTable, row permutation)
        self._ws = None
        self.device = None

    # ------------------------------------------------------------------------------------------ weights
    def set_precision(self, mode: str):
        npass = {"bf16x3": 3, "fp32": 3, "bf16": 1}[mode]
        if npass != self.npass:
            self.npass = npass
            self._plans.clear()

    def _recipes(self) -> "RecipeBook":
        """Declarative description of every operand the kernels consume: which parameter (reference layout) goes where in
        which packed matrix / vector.  ``refresh_weights`` turns it into the device table of ``wd_repack_multi``."""
        m = self.model
        R = RecipeBook()
        film_w = []
        self.film_off = {}
        off = 0
        cin_conv = m.input_blocks[0][0]
        self.kpad_in = ((9 * cin_conv.in_channels + 31) // 32) * 32
        R.matrix("in.w", cin_conv.out_channels, self.kpad_in).fwd(cin_conv.weight)
        R.vector("in.b", cin_conv.bias)
        R.vector("in.w.f32", cin_conv.weight)  # the direct first convolution reads the parameter layout itself
        R.linear("te0", m.time_embed[0])
        R.linear("te2", m.time_embed[2])
        if m.num_classes is not None:
            R.vector("label", m.label_emb.weight)
        we = m.word_emb
        cd = we.embedding.weight.shape[1]
        R.vector("we.table", we.embedding.weight)
        qkv = (we.attention.linear_query, we.attention.linear_key, we.attention.linear_value)
        R.matrix("we.qkv.w", 3 * cd, cd)
        R.vector_cat("we.qkv.b", [l.bias for l in qkv])
        for i, l in enumerate(qkv):
            R["we.qkv.w"].fwd(l.weight, row_off=i * cd)
        kv_w = []
        self.kv_off = {}
        kvo = 0
        for name, mod in self._walk():
            if isinstance(mod, ResBlockParams):
                R.vector(name + ".gn1.g", mod.in_layers[0].weight)
                R.vector(name + ".gn1.b", mod.in_layers[0].bias)
                R.matrix(name + ".c1.w", mod.cout, 9 * mod.cin).fwd(mod.in_layers[2].weight)
                R.vector(name + ".c1.b", mod.in_layers[2].bias)
                R.vector(name + ".gn2.g", mod.out_layers[0].weight)
                R.vector(name + ".gn2.b", mod.out_layers[0].bias)
                if mod.cin != mod.cout:
                    # the 1x1 skip projection is a second K segment of the last 3x3 GEMM; the biases add
                    R.matrix(name + ".c2.w", mod.cout, 9 * mod.cout + mod.cin).fwd(mod.out_layers[3].weight) \
                        .fwd(mod.skip_connection.weight, col_off=9 * mod.cout)
                    R.vector(name + ".c2.b", mod.out_layers[3].bias, mod.skip_connection.bias)
                else:
                    R.matrix(name + ".c2.w", mod.cout, 9 * mod.cout).fwd(mod.out_layers[3].weight)
                    R.vector(name + ".c2.b", mod.out_layers[3].bias)
                film_w.append(mod.emb_layers[1])
                self.film_off[name] = off
                off += mod.cout
            elif isinstance(mod, (DownsampleParams, UpsampleParams)):
                conv = mod.op if isinstance(mod, DownsampleParams) else mod.conv
                R.matrix(name + ".w", mod.cout, 9 * mod.cin).fwd(conv.weight)
                R.vector(name + ".b", conv.bias)
                if isinstance(mod, UpsampleParams) and self._up_phases_ok(mod):
                    # the four phase matrices [cout][4 taps x cin] from a derived tensor (the summed taps), refreshed before every repack
                    key = name + ".wph"
                    if key not in self._derived or self._derived[key][0].device != conv.weight.device:
                        self._derived[key] = (torch.empty((4, 4, mod.cout, mod.cin), dtype=torch.float32, device=conv.weight.device),
                                              (lambda cv=conv: upsample_phase_weights(cv.weight)))
                    wph = self._derived[key][0]
                    for ph in range(4):
                        r = R.matrix(f"{name}.wph{ph}", mod.cout, 4 * mod.cin)
                        for t in range(4):
                            r.fwd(wph[ph, t], col_off=t * mod.cin)
            elif isinstance(mod, SpatialTransformerParams):
                inner = mod.heads * mod.d_head
                R.vector(name + ".gn.g", mod.norm.weight)
                R.vector(name + ".gn.b", mod.norm.bias)
                R.matrix(name + ".pi.w", inner, mod.ch).fwd(mod.proj_in.weight)
                R.vector(name + ".pi.b", mod.proj_in.bias)
                R.matrix(name + ".po.w", mod.ch, inner).fwd(mod.proj_out.weight)
                R.vector(name + ".po.b", mod.proj_out.bias)
                for d, tb in enumerate(mod.transformer_blocks):
                    p = f"{name}.tb{d}"
                    for ln in ("norm1", "norm2", "norm3"):
                        R.vector(f"{p}.{ln}.g", getattr(tb, ln).weight)
                        R.vector(f"{p}.{ln}.b", getattr(tb, ln).bias)
                    if self.variant == "phosc":
                        R.matrix(p + ".a1.qkv.w", 3 * inner, inner)
                        for i, l in enumerate((tb.attn1.to_q, tb.attn1.to_k, tb.attn1.to_v)):
                            R[p + ".a1.qkv.w"].fwd(l.weight, row_off=i * inner)
                        cross = [("a2", tb.attn2)]
                    else:
                        R.matrix(p + ".a1.q.w", inner, inner).fwd(tb.attn1.to_q.weight)
                        cross = [("a1", tb.attn1), ("a2", tb.attn2)]
                    R.matrix(p + ".a2.q.w", inner, inner).fwd(tb.attn2.to_q.weight)
                    for tag, at in cross:
                        kv_w.append(at)
                        self.kv_off[f"{p}.{tag}"] = kvo
                        kvo += 2 * at.to_k.weight.shape[0]
                        # fp32 copies for the folded cross-attention (wd_xattn_fold)
                        R.vector(f"{p}.{tag}.q.f32", at.to_q.weight)
                        R.vector(f"{p}.{tag}.o.f32", at.to_out[0].weight)
                    for tag, at in (("a1", tb.attn1), ("a2", tb.attn2)):
                        R.linear(f"{p}.{tag}.o", at.to_out[0])
                    ffi = tb.ff.net[2].in_features
                    g = geglu_tile(ffi) % 1000 // 2
                    R.matrix(p + ".ff1.w", 2 * ffi, inner).fwd(tb.ff.net[0].proj.weight, g=g)
                    R.vector(p + ".ff1.b", tb.ff.net[0].proj.bias, g=g)
                    R.linear(p + ".ff2", tb.ff.net[2])
                    if N.lib().wd_ff_supported(inner, ffi):
                        # the fused feed-forward (csrc/wd_ff.hip): x | gate rows in blocks of 16, one MFMA tile each
                        R.matrix(p + ".ff1f.w", 2 * ffi, inner).fwd(tb.ff.net[0].proj.weight, g=16)
                        R.vector(p + ".ff1f.b", tb.ff.net[0].proj.bias, g=16)
                if self.fold_proj:
                    # the last block's ff.net[2] and proj_out as one product: derived tensors (W32, b32), refreshed before every repack
                    tb = mod.transformer_blocks[-1]
                    lin, po = tb.ff.net[2], mod.proj_out
                    ffi, dev = lin.in_features, po.weight.device
                    key = name + ".w32"
                    if key not in self._derived or self._derived[key][0].device != dev:
                        w32 = torch.empty((mod.ch, ffi), dtype=torch.float32, device=dev)
                        b32 = torch.empty((mod.ch,), dtype=torch.float32, device=dev)

                        def fold(lin=lin, po=po, w32=w32, b32=b32, rows=mod.ch, k=inner, cols=ffi):
                            st = torch.cuda.current_stream(w32.device).cuda_stream
                            N.check(self.lib.wd_linear_fold(po.weight.data_ptr(), lin.weight.data_ptr(), _ptr(lin.bias), _ptr(po.bias),
                                                            rows, k, cols, w32.data_ptr(), b32.data_ptr(), st), "wd_linear_fold")

                        self._derived[key] = (w32, fold)          # (writes both tensors in place)
                        self._derived[name + ".b32"] = (b32, None)
                    w32, b32 = self._derived[key][0], self._derived[name + ".b32"][0]
                    R.matrix(name + ".po32.w", mod.ch, ffi + inner).fwd(w32).fwd(po.weight, col_off=ffi)   # [W32 | W3]
                    R.vector(name + ".b32", b32)
                    if inner == mod.ch and N.lib().wd_ff_supported(inner, ffi):
                        R.matrix(name + ".w32.w", mod.ch, ffi).fwd(w32)   # the fused kernel's image in w2's place
        self.film_total = off
        self.kv_total = kvo
        ted = m.time_embed[2].out_features
        R.matrix("film.w", off, ted)
        R.vector_cat("film.b", [l.bias for l in film_w])
        r0 = 0
        for l in film_w:
            R["film.w"].fwd(l.weight, row_off=r0)
            r0 += l.weight.shape[0]
        if kv_w:
            R.matrix("kv.w", kvo, kv_w[0].to_k.weight.shape[1])
            r0 = 0
            for at in kv_w:
                for l in (at.to_k, at.to_v):
                    R["kv.w"].fwd(l.weight, row_off=r0)
                    r0 += l.weight.shape[0]
        self._film_mods, self._kv_mods = film_w, kv_w
        R.vector("out.gn.g", m.out[0].weight)
        R.vector("out.gn.b", m.out[0].bias)
        R.matrix("out.w", m.out[2].out_channels, 9 * m.out[2].in_channels).fwd(m.out[2].weight)
        R.vector("out.b", m.out[2].bias)
        R.vector("out.w.f32", m.out[2].weight)  # the fused GroupNorm + SiLU + 3x3 kernel reads the parameter layout itself
        return R

    def _walk(self):
        """(name, module) of every block layer in execution order."""
        m = self.model
        for i, blk in enumerate(m.input_blocks):
            for j, mod in enumerate(blk):
                yield f"in{i}.{j}", mod
        for j, mod in enumerate(m.middle_block):
            yield f"mid.{j}", mod
        for i, blk in enumerate(m.output_blocks):
            for j, mod in enumerate(blk):
                yield f"out{i}.{j}", mod

    def _signature(self):
        # the module-tree walk of ``model.parameters()`` costs ~0.35 ms for the 264 tensors, 10x the rest of this function:
        # the list is kept until some module of the process registers a Parameter (object identity can only change then)
        if self._ps is None or self._ps_gen != _PARAM_GEN[0]:
            self._ps, self._ps_gen = list(self.model.parameters()), _PARAM_GEN[0]
        ps = self._ps
        return (sum(p._version for p in ps) + (_NATIVE_WRITES[0] << 32), hash(tuple(p.data_ptr() for p in ps)), str(ps[0].device))

    def refresh_weights(self, force: bool = False):
        """Re-derives the packed operands from the parameters when they changed (optimiser step, load_state_dict,
        .to(device)): one ``wd_repack_multi`` launch over a device table built once per parameter placement."""
        sig = self._signature()
        if not force and sig == self._sig:
            return
        dev = next(self.model.parameters()).device
        if dev.type != "cuda":
            raise N.NativeError("worddiffusion_amd runs on an MI355X only: move the model to cuda "
                                "(there is no CPU / eager fallback)")
        if self.device is not None and dev != self.device:
            self._w.clear()
            self._w3.clear()
            self._wf.clear()
            self._w3_meta.clear()
            self._plans.clear()
            self._tabs.clear()
            self._ws = None
            self._pack = None
        self.device = dev
        if self._pack is None or self._pack[0] != sig[1:]:
            book = self._recipes()
            for p in self.model.parameters():
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise N.NativeError("parameters must be contiguous fp32 (the reference never retypes them, unet.py:415)")
            for name, r in book.items():
                if name not in self._w:
                    self._w[name] = (torch.zeros((2, r.rows, r.cols), dtype=torch.bfloat16, device=dev) if r.planes
                                     else torch.zeros(r.shape, dtype=torch.float32, device=dev))
            table, chunks, n = book.device_table(self.lib, self._w, dev, self._wf)
            # (the fragment-major images the table does not write itself are re-made from the planes below)
            self._pack = (sig[1:], table, chunks, n, [k for k in self._wf if k not in book or not book.frag_ok(book[k])])
        _, table, chunks, n, wf_left = self._pack
        stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.no_grad():
            for buf, fn in self._derived.values():
                r = fn() if fn is not None else None   # (None: a native launch wrote the tensors in place)
                if r is not None:
                    buf.copy_(r)
        N.check(self.lib.wd_repack_multi(table.data_ptr(), n, chunks, stream), "wd_repack_multi")
        for name in wf_left:
            self._pack_wf(name, self._wf[name], stream)
        with torch.no_grad():
            for name, meta in self._w3_meta.items():
                self._w3[name].copy_(slab_order(self._w[name], *meta))
            if "freqs" not in self._w and hasattr(self.model, "word_emb"):  # (the VAE decoder engine has neither)
                half = self.model.model_channels // 2
                freqs = torch.exp(-math.log(10000) * torch.arange(0, half, dtype=torch.float32) / half)
                self._w["freqs"] = freqs.to(dev)
                self._w["pe"] = self.model.word_emb.positional_encoding.to(dev).contiguous()
        self._sig = sig

    def _pack_wf(self, name, wf, stream):
        wp = self._w[name]
        N.check(self.lib.wd_gemm_pack_w(wp[0].data_ptr(), wp[1].data_ptr(), wp.shape[1], wp.shape[2], wf[0].data_ptr(),
                                        wf[1].data_ptr(), stream), "wd_gemm_pack_w")

    # ------------------------------------------------------------------------------------------ helpers
    def _table(self, h, w, mode) -> GatherTable:
        key = (h, w, mode)
        if key not in self._tabs:
            tab, ho, wo = conv_gather_table(h, w, mode)
            self._tabs[key] = GatherTable(torch.from_numpy(tab).to(self.device), ho, wo, tab, *gather_hint(mode, w, wo))
        return self._tabs[key]

    def _f32(self, P: Plan, *shape):
        t = torch.empty(shape, dtype=torch.float32, device=self.device)
        P.keep.append(t)
        return t

    def _planes(self, P: Plan, rows, ld):
        t = torch.zeros((2, rows, ld), dtype=torch.bfloat16, device=self.device)
        P.keep.append(t)
        return t

    def _hilo(self, planes: Optional[torch.Tensor], byte_off: int = 0):
        """(hi, lo) pointers of operand planes [2, rows, ld] for a kernel: the low plane exists in three-pass mode only (lo is
        None otherwise); (None, None) for no planes at all."""
        if planes is None:
            return None, None
        return planes[0].data_ptr() + byte_off, (planes[1].data_ptr() + byte_off if self.npass == 3 else None)

    def _src(self, planes: torch.Tensor, c: int, ntaps: int = 1, gather: Optional[GatherTable] = None,
             hw_src: int = 0, col_off: int = 0) -> Src:
        s = N.WdSrc()
        s.hi = planes[0].data_ptr() + 2 * col_off
        s.lo = planes[1].data_ptr() + 2 * col_off
        s.gather = gather.dev.data_ptr() if gather is not None else None
        s.ld, s.c, s.ntaps, s.hw_src = planes.shape[2], c, ntaps, hw_src
        return Src(s, gather)

    def _gemm_args(self, srcs: List[Src], m, n, hw_out, a32=None) -> N.WdGemmArgs:
        """The part of wd_gemm_args every kernel form shares and wd_gemm_check's answer turns on first: the sources, the shape,
        the passes and the fp32 map src[0] stands for (a32, see ``_gemm``)."""
        a = N.WdGemmArgs()
        for i, s in enumerate(srcs):
            a.src[i] = s.raw
        a.nsrc, a.npass = len(srcs), self.npass
        a.m, a.n, a.ktot, a.hw_out = m, n, sum(s.raw.ntaps * s.raw.c for s in srcs), hw_out
        if a32 is not None:
            self._set_a32(a, *a32)
        return a

    def _gemm(self, ops, what, srcs: List[Src], wname, m, hw_out, bias=None, rowvec=None, rowvec_ld=0, resid=None,
              resid_ld=0, resid_rows=None, act=N.ACT_NONE, out_f32=None, out_ld=0, out_pl=None, n=None, tile=0,
              w_row_off=0, want_stats=False, a32=None, ln=None, w_groups=None) -> GemmOp:
        """a32 = (Act, norm name, eps, silu): src[0] is that fp32 map, normalised while it is staged (wd_gemm_args.a32*).
        ln: name of the LayerNorm whose output the epilogue also writes, as new planes ``GemmOp.ln_pl``, where wd_gemm takes it
        (wd_gemm_args.ln_*; None otherwise).  w_groups = (count, stride): weight groups (wd_gemm_args.w_ngroups).
        What wd_gemm can run is wd_gemm_check's answer; the tests written here are policy."""
        wp = self._w[wname]
        ktot = wp.shape[2]
        nrows = wp.shape[1] if n is None else n
        a = self._gemm_args(srcs, m, nrows, hw_out, a32)
        assert ktot == a.ktot, (what, ktot, [(s.raw.ntaps, s.raw.c) for s in srcs])
        a.w_hi = wp[0].data_ptr() + 2 * w_row_off * ktot
        a.w_lo = wp[1].data_ptr() + 2 * w_row_off * ktot
        a.bias = _ptr(bias)
        a.rowvec, a.rowvec_ld = rowvec, rowvec_ld
        a.resid, a.resid_ld, a.resid_rows = resid, resid_ld, resid_rows
        a.act = act
        a.out_f32, a.out_ld = _ptr(out_f32), out_ld
        if out_pl is not None:
            a.out_hi, a.out_lo, a.out_pl_ld = out_pl[0].data_ptr(), out_pl[1].data_ptr(), out_pl.shape[2]
        if w_groups is not None:
            a.w_ngroups, a.w_group_stride = w_groups
        a.tile = tile
        if self._ws is None:
            self._ws = torch.empty(128 * 128 * 160 * 8, dtype=torch.float32, device=self.device)  # 84 MB split-K scratch
        a.ksplit, a.ws, a.ws_floats = 0, self._ws.data_ptr(), self._ws.numel()
        self._give_tickets(a, m, nrows)
        form = self._gemm_form(a, srcs, whole_w=w_row_off == 0 and n is None, w_row_off=w_row_off)
        assert (a32 is None and w_groups is None) or form.kind == "wdirect", what
        self._apply_form(a, form, wname, srcs)
        ln_pl = self._fuse_ln(a, ln) if ln is not None else None
        stats = self._fuse_stats(a, form) if want_stats else None
        self._cur_plan.keep.append(a)
        ops.append((self.lib.wd_gemm, (C.byref(a),), what))
        return GemmOp(a, stats, ln_pl)

    def _gemm_form(self, a, srcs: List[Src], whole_w: bool, w_row_off: int) -> GemmForm:
        """The kernel form of the GEMM ``a`` (sources, shape, epilogue and tile filled in; whole_w: it reads the whole weight
        matrix), the first of the candidates below that applies.  Each candidate is policy - where a form is worth taking; whether
        wd_gemm can run it is wd_gemm_check's answer (``_legal``).  WDIFF_SLAB / WDIFF_CONV3 (experimental build): the slab-order
        kernel goes first, and WDIFF_CONV3 keeps every GEMM off the fragment-major forms."""
        s0, t0 = srcs[0].raw, srcs[0].tab
        s1 = srcs[1].raw if len(srcs) > 1 else None
        m, n, hw_out = a.m, a.n, a.hw_out
        conv = s0.ntaps == 9 and t0 is not None
        same_w = t0.same_w if conv else 0
        identity_tail = s1 is None or (s1.ntaps == 1 and not s1.gather)
        auto = a.act == N.ACT_NONE and a.tile == 0
        # 1. slab-order weights (w_layout 1): 128-row panels whose source slab stays in LDS - only worth it when they fill the chip
        if self.use_slab and w_row_off == 0 and identity_tail:
            span = slab_span(t0.host if t0 is not None else None, hw_out, s0.hw_src, m)
            if 0 < span <= 192 and ((m + 127) // 128) * max(1, n // 160) >= 96:
                return GemmForm("slab-order", dict(w_layout=1, slab_rows=span))
        # fragment-major weights (w_layout 3): only for whole matrices with the auto tile and no activation
        if whole_w and auto and not self.use_conv3:
            # 2. 64 x 320 tiles, weights straight to registers.  (The K-cut layers of the 4 x 16 level stay on the LDS-staged kernel:
            # this one is 5 % faster on their long loops in isolation and 2 % slower inside the step - hence the chip-fill rule)
            if self.use_wdirect and wdirect_fills_chip(m, n):
                fields = dict(w_layout=3, tile=64320, slab_rows=same_w)
                if self._legal(a, apply=False, **fields):
                    return GemmForm("wdirect", fields)
            # 3. 3x3 layers over 64-position samples (the 4 x 16 level): 64 x 80 tiles with all of K inside the workgroup
            # (wd_gemmq_kernel) instead of a K cut over workgroups + combine launch, where that grid holds 128 to 512 tiles.
            # slab_rows: the image width of the 3x3 table - the OUTPUT width for a stride-2 table
            if self.use_smallmap and hw_out == 64 and 128 <= (m // 64) * (n // 80) <= 512:
                fields = dict(w_layout=3, tile=64080, slab_rows=(t0.down_w or t0.same_w) if conv else 0)
                if self._legal(a, apply=False, **fields):
                    return GemmForm("whole-k", fields)
        # 4. the generic kernels, wd_gemm's own choice.  w_layout 2 for a 3x3 same-convolution is a hint: it lets the kernel compute
        # the source-row table (WDIFF_CONV3=1 also selects the row-shared-taps kernel for it)
        if same_w and s0.c % 64 == 0 and auto and identity_tail and (s1 is None or s1.c % 64 == 0):
            return GemmForm("generic", dict(w_layout=2, slab_rows=same_w))
        return GemmForm("generic", {})

    def _apply_form(self, a, form: GemmForm, wname, srcs: List[Src]):
        """Sets the form's fields on ``a``, points it at the weight image the form reads (fragment-major / slab order: made on first
        use) and passes the engine's own WDIFF_GEMMW_SLAB / WDIFF_EPI_BATCH with the forms those switches bear on."""
        for k, v in form.fields.items():
            setattr(a, k, v)
        if form.kind in ("wdirect", "whole-k"):
            wf = self._wfrag(wname)
            a.w_hi, a.w_lo = wf[0].data_ptr(), wf[1].data_ptr()
            if form.kind == "wdirect" and self.gemmw_slab is not None:
                a.dbg |= N.GEMMW_SLAB_ON if self.gemmw_slab else N.GEMMW_SLAB_OFF
            if self.epi_batch is not None:
                a.dbg |= N.EPI_BATCH_ON if self.epi_batch else N.EPI_BATCH_OFF
        elif form.kind == "slab-order":
            meta = (srcs[0].raw.ntaps, srcs[0].raw.c, srcs[1].raw.c if len(srcs) > 1 else 0)
            if wname not in self._w3:
                self._w3[wname] = slab_order(self._w[wname], *meta)
                self._w3_meta[wname] = meta
            assert self._w3_meta[wname] == meta, wname
            w3 = self._w3[wname]
            a.w_hi, a.w_lo = w3[0].data_ptr(), w3[1].data_ptr()

    def _fuse_ln(self, a, ln: str) -> Optional[torch.Tensor]:
        """The LayerNorm ``ln`` of the result in the GEMM's own epilogue, where wd_gemm takes it: the planes it then writes."""
        if not self.fuse_ln or self.use_slab:  # (WDIFF_SLAB=1 runs keep the LayerNorm launches)
            return None
        pl = torch.zeros((2, a.m, a.n), dtype=torch.bfloat16, device=self.device)
        if not self._legal(a, out_hi=pl[0].data_ptr(), out_lo=pl[1].data_ptr(), out_pl_ld=a.n, ln_gamma=self._w[ln + ".g"].data_ptr(),
                           ln_beta=self._w[ln + ".b"].data_ptr(), ln_eps=1e-5):
            return None
        self._cur_plan.keep.append(pl)
        return pl

    def _fuse_stats(self, a, form: GemmForm) -> Optional[tuple]:
        """The GroupNorm statistics of the result from the GEMM's epilogue, where wd_gemm takes them: ``Act.stats`` of the output.
        (The consumer's GroupNorm has 32 groups; the statistics layout is kept to sample sizes that are a multiple of the 128-row
        panel or exactly 64 rows, and off the experimental slab kernel.)"""
        m, n, hw_out = a.m, a.n, a.hw_out
        if not (self.fuse_stats and n % 32 == 0 and (hw_out % 128 == 0 or hw_out == 64) and form.kind != "slab-order"):
            return None
        cpg = n // 32
        r = self._resolved(a, stat_part=a.ws, stat_cpg=cpg)  # (a placeholder for the partials: the count depends on the tile)
        if r is None:
            return None
        nchunk = max(1, hw_out // (r.tile // 1000))  # (the statistics are kept per row panel of the tile)
        part = torch.zeros((m // hw_out, nchunk, 32, 2), dtype=torch.float64, device=self.device)
        self._cur_plan.keep.append(part)
        a.stat_part, a.stat_cpg = part.data_ptr(), cpg
        return part, nchunk, cpg

    def _resolved(self, a, **fields) -> Optional[N.WdGemmArgs]:
        """``a`` with ``fields`` set (on a copy) as wd_gemm would launch it, or None where wd_gemm refuses it (wd_gemm_check)."""
        b = N.WdGemmArgs.from_buffer_copy(a)
        for k, v in fields.items():
            setattr(b, k, v)
        out = N.WdGemmArgs()
        return out if self.lib.wd_gemm_check(C.byref(b), C.byref(out)) == N.WD_OK else None

    def _legal(self, a, apply=True, **fields) -> bool:
        """Does wd_gemm take ``a`` with ``fields`` set?  If it does (and ``apply``), they are set on ``a`` itself."""
        if self._resolved(a, **fields) is None:
            return False
        if apply:
            for k, v in fields.items():
                setattr(a, k, v)
        return True

    def _set_a32(self, a, x32: "Act", gname, eps, silu):
        part, nchunk, pc = x32.stats
        a.a32, a.a32_ld, a.a32_part = x32.t.data_ptr(), x32.c, part.data_ptr()
        a.a32_nchunk, a.a32_pcpg, a.a32_cpg = nchunk, pc, x32.c // 32
        a.a32_gamma, a.a32_beta = self._w[gname + ".g"].data_ptr(), self._w[gname + ".b"].data_ptr()
        a.a32_eps, a.a32_silu = float(eps), int(silu)

    def _wdirect_ok(self, srcs, m, n, hw_out, a32=None, **fields) -> bool:
        """Would wd_gemm run a GEMM over ``srcs`` into m x n as the 64 x 320 weights-to-registers kernel (with a32 / ``fields``)?
        Asked before the GEMM is planned; weights and output are placeholders (wd_gemm_check reads no memory)."""
        a = self._gemm_args(srcs, m, n, hw_out, a32)
        a.w_layout, a.tile = 3, 64320
        a.w_hi = a.w_lo = a.out_f32 = 16
        a.out_ld = n  # (a dense m x n output: wd_gemm_check refuses a pitch narrower than the width)
        return self._legal(a, apply=False, **fields)

    def _give_tickets(self, a, m, n):
        """Arrival counters for the in-launch split-K combine of one wd_gemm launch: a range of its own inside a zeroed
        per-plan buffer (zero before and after every launch; only small grids ever split, so only they get one)."""
        ntick = ((m + 63) // 64) * ((n + 63) // 64)
        if ntick > 2048:
            return
        P = self._cur_plan
        if P.tickets is None or P.ticket_off + ntick > P.tickets.numel():
            P.tickets, P.ticket_off = torch.zeros(1 << 16, dtype=torch.int32, device=self.device), 0
            P.keep.append(P.tickets)
        a.tickets, a.ntickets = P.tickets.data_ptr() + 4 * P.ticket_off, ntick
        P.ticket_off += ntick

    def _gn(self, P, ops, what, srcs: List[Act], gname, eps, silu, want_raw=False, dropout=None):
        """GroupNorm over the channel concat of ``srcs`` -> planes [M, sum c] (+ raw planes).  dropout: the wd_dropout of a training
        ResBlock's second norm (one source) - the norm then takes the wd_gn_apply_dropout launch and is never fused into its producer."""
        B = self._B
        h, w = srcs[0].h, srcs[0].w
        hw = h * w
        ctot = sum(s.c for s in srcs)
        cpg = ctot // 32
        has_perm = any(s.perm is not None for s in srcs)
        if has_perm and not (len(srcs) == 2 and srcs[1].perm is None and self.fuse_gn2 and not any(s.c % cpg for s in srcs)):
            # (not reachable from a constructor argument: _resample plans the phase form only where _phase_map_readable says this
            # GroupNorm takes it)
            raise NotImplementedError(f"{what}: a phase-major map (Upsample) is read by the two-source GroupNorm of a decoder block only")
        if any(s.c % cpg for s in srcs):
            # groups straddle the concat boundary: materialise the concat (never the case at 320+320 channels)
            cat = self._f32(P, B * hw, ctot)
            coff = 0
            for s in srcs:
                ops.append((self.lib.wd_copy2d, (cat.data_ptr() + 4 * coff, 4 * ctot, s.t.data_ptr(), 4 * s.c, 4 * s.c,
                                                 B * hw), what + ":concat"))
                coff += s.c
            srcs = [Act(cat, ctot, h, w)]
        pl = self._planes(P, B * hw, ctot)
        raw = self._planes(P, B * hw, ctot) if want_raw else None
        for s in srcs:
            self._gn_stats(P, ops, what, s)
        coff = 0
        gam, bet = self._w[gname + ".g"], self._w[gname + ".b"]
        todo = []  # (source, part, nchunk, pc, coff) of the sources that need an apply launch
        for s in srcs:
            part, nchunk, pc = s.stats
            assert cpg % pc == 0, (what, cpg, pc)
            if nchunk > 8:
                # many chunks per sample (large images): fold them once here, not in every workgroup of wd_gn_apply
                ngs = s.c // pc
                folded = torch.empty((B, 1, ngs, 2), dtype=torch.float64, device=self.device)
                P.keep.append(folded)
                ops.append((self.lib.wd_gn_fold_chunks, (part.data_ptr(), B, nchunk, ngs, folded.data_ptr()), what + ":fold chunks"))
                part, nchunk = folded, 1
                s.stats = (part, nchunk, pc)
            # (_gn_in_combine: the producer is a K-cut GEMM whose combine tiles (64 rows x 40 columns) hold whole (sample, group)
            # blocks - its combine launch normalises the rows it has just summed and writes these planes)
            if has_perm or dropout is not None or not self._gn_in_combine(s, raw, gam, bet, eps, silu, cpg, pl, coff):
                todo.append((s, part, nchunk, pc, coff))
            coff += s.c
        hi, lo = self._hilo(pl)
        rhi, rlo = self._hilo(raw)
        if len(todo) == 2 and self.fuse_gn2:  # [h | skip] of a decoder block: one launch for both halves of the concat
            (sa, pa, na, pca, ca), (sb, pb, nb_, pcb, cb) = todo
            ops.append((self.lib.wd_gn_apply2,
                        (sa.t.data_ptr(), sa.c, sa.c, pa.data_ptr(), na, pca, ca, sb.t.data_ptr(), sb.c, sb.c, pb.data_ptr(), nb_, pcb, cb,
                         B, hw, cpg, gam.data_ptr(), bet.data_ptr(), eps, int(silu), hi, lo, ctot, rhi, rlo,
                         sa.perm.data_ptr() if sa.perm is not None else None),
                        what + ":apply"))
        elif dropout is not None:
            assert not has_perm and len(srcs) == 1, what
            (s, part, nchunk, pc, c0), = todo
            ops.append((self.lib.wd_gn_apply_dropout,
                        (s.t.data_ptr(), s.c, B, hw, s.c, cpg, part.data_ptr(), nchunk, pc, gam.data_ptr(), bet.data_ptr(), eps,
                         int(silu), hi, lo, ctot, c0, rhi, rlo, C.byref(dropout)), what + ":apply+dropout"))
        else:
            assert not has_perm, what
            for s, part, nchunk, pc, c0 in todo:
                ops.append((self.lib.wd_gn_apply,
                            (s.t.data_ptr(), s.c, B, hw, s.c, cpg, part.data_ptr(), nchunk, pc, gam.data_ptr(), bet.data_ptr(), eps,
                             int(silu), hi, lo, ctot, c0, rhi, rlo), what + ":apply"))
        return pl, raw

    def _gn_stats(self, P, ops, what, s: Act):
        """GroupNorm statistics of a map whose producer left none: one pass over the tensor (32 groups of c/32 channels)."""
        if s.stats is None:
            B, hw = self._B, s.h * s.w
            nchunk = self.lib.wd_gn_nchunk(hw)
            pc = s.c // 32
            part = torch.empty((B, nchunk, 32, 2), dtype=torch.float64, device=self.device)
            P.keep.append(part)
            ops.append((self.lib.wd_gn_stats, (s.t.data_ptr(), s.c, B, hw, s.c, pc, part.data_ptr()), what + ":stats"))
            s.stats = (part, nchunk, pc)
        return s.stats

    def _gn_in_consumer(self, P, ops, what, srcs: List[Act], want_raw, M, hw, ncols, taps=1, gather=None) -> bool:
        """Can the convolution that consumes this GroupNorm (``what``: also the norm's name) apply it itself (wd_gemm_args.a32*)?
        One fp32 source with known (or computable) statistics, a consumer that takes the 64 x 320 weights-to-registers kernel
        (``_wdirect_ok``: wd_gemm_check on its args with the a32 fields).
        Measured at B = 64: a 1x1 consumer (proj_in: five stages, no SiLU) loses nothing and saves the wd_gn_apply launch; a 3x3
        consumer normalises and activates every element nine times (once per tap) and runs ~30 us longer per launch than the
        10 us launch it saves (step 2.095 -> 2.137 ms with all of them on) - WDIFF_FUSE_GN_IN=2 switches those on anyway."""
        if not (self.fuse_gn_in and self.use_wdirect and len(srcs) == 1 and not want_raw and not self.use_conv3):
            return False
        if taps > 1 and self.fuse_gn_in < 2:
            return False
        if not wdirect_fills_chip(M, ncols):
            return False
        s = srcs[0]
        self._gn_stats(P, ops, what, s)
        return self._wdirect_ok([self._src32(s, taps, gather, hw)], M, ncols, hw, a32=(s, what, 0.0, False))

    def _src32(self, x: Act, ntaps=1, gather: Optional[GatherTable] = None, hw_src=0) -> Src:
        """src[0] of a GEMM that reads the fp32 map itself (a32): channel count, taps and gather table only."""
        s = N.WdSrc()
        s.hi, s.lo, s.gather = None, None, gather.dev.data_ptr() if gather is not None else None
        s.ld, s.c, s.ntaps, s.hw_src = x.c, x.c, ntaps, hw_src
        return Src(s, gather)

    def _gn_in_combine(self, s: Act, raw, gam, bet, eps, silu, cpg, pl, coff) -> bool:
        """Let the GEMM that produced ``s`` apply this GroupNorm as it combines its K slices (or in its own epilogue where it holds
        all of K) and write columns coff.. of the planes ``pl`` (wd_gemm_args.gn_*), where wd_gemm_check accepts that.  The
        producer must write exactly this tensor, with no planes of its own yet."""
        pr = s.prod
        if pr is None or not isinstance(pr, N.WdGemmArgs) or not self.fuse_gn or raw is not None or self.use_conv3:
            return False
        if pr.out_f32 != s.t.data_ptr() or pr.out_hi or pr.gn_gamma or pr.n != s.c:
            return False
        hi, lo = self._hilo(pl, 2 * coff)
        return self._legal(pr, gn_gamma=gam.data_ptr() + 4 * coff, gn_beta=bet.data_ptr() + 4 * coff, gn_eps=float(eps),
                           gn_silu=int(silu), gn_cpg=cpg, out_hi=hi, out_lo=lo, out_pl_ld=pl.shape[2])

    def _ln(self, P, ops, what, x: torch.Tensor, rows, c, name):
        pl = self._planes(P, rows, c)
        ops.append((self.lib.wd_layernorm,
                    (x.data_ptr(), c, rows, c, self._w[name + ".g"].data_ptr(), self._w[name + ".b"].data_ptr(), 1e-5,
                     *self._hilo(pl), c), what))
        return pl

    # ------------------------------------------------------------------------------------------ blocks
    def _resblock(self, P, name, mod: ResBlockParams, srcs: List[Act]) -> Act:
        ops = P.step
        B = self._B
        h, w = srcs[0].h, srcs[0].w
        hw, M = h * w, B * h * w
        cin, cout = mod.cin, mod.cout
        assert cin == sum(s.c for s in srcs)
        tab = self._table(h, w, "same")
        need_raw = cin != cout
        h1 = self._f32(P, M, cout)
        if self._gn_in_consumer(P, ops, name + ".gn1", srcs, need_raw, M, hw, cout, taps=9, gather=tab):
            s1, in1 = self._src32(srcs[0], 9, tab, hw), (srcs[0], name + ".gn1", 1e-5, True)
            raw = None
        else:
            a1, raw = self._gn(P, ops, name + ".gn1", srcs, name + ".gn1", 1e-5, True, want_raw=need_raw)
            s1, in1 = self._src(a1, cin, 9, tab, hw), None
        g1 = self._gemm(ops, name + ".conv1", [s1], name + ".c1.w", M, hw,
                        bias=self._w[name + ".c1.b"], rowvec=self._film.data_ptr() + 4 * self.film_off[name],
                        rowvec_ld=self.film_total, out_f32=h1, out_ld=cout, want_stats=True, a32=in1)
        h1a = Act(h1, cout, h, w, g1.stats, prod=g1.args)
        if self._gn_in_consumer(P, ops, name + ".gn2", [h1a], False, M, hw, cout, taps=9, gather=tab):
            s2, in2 = self._src32(h1a, 9, tab, hw), (h1a, name + ".gn2", 1e-5, True)
        else:
            a2, _ = self._gn(P, ops, name + ".gn2", [h1a], name + ".gn2", 1e-5, True)
            s2, in2 = self._src(a2, cout, 9, tab, hw), None
        out = self._f32(P, M, cout)
        if need_raw:
            g2 = self._gemm(ops, name + ".conv2+skip", [s2, self._src(raw, cin)],
                            name + ".c2.w", M, hw, bias=self._w[name + ".c2.b"], out_f32=out, out_ld=cout,
                            want_stats=True, a32=in2)
        else:
            g2 = self._gemm(ops, name + ".conv2", [s2], name + ".c2.w", M, hw,
                            bias=self._w[name + ".c2.b"], resid=srcs[0].t.data_ptr(), resid_ld=cout, out_f32=out,
                            out_ld=cout, want_stats=True, a32=in2)
        return Act(out, cout, h, w, g2.stats, prod=g2.args)

    def _up_phases_ok(self, mod) -> bool:
        """Is the phase form of an Upsample switched on (the 64 x 320 weights-to-registers kernel with weight groups; whether it
        takes a given shape, ``_resample`` asks wd_gemm_check)?"""
        return (getattr(self, "use_up_phases", False) and self.use_wdirect and self.fuse_gn2 and self.npass == 3 and not self.use_slab and
                not self.use_conv3)

    def _phase_map_readable(self, cout: int, cskip: Optional[int]) -> bool:
        """Can the consumer of an Upsample's output read it phase-major?  Only the two-source GroupNorm launch of the decoder block
        behind it does (wd_gn_apply2 with a row permutation, ``_gn``): the block normalises [Upsample output | skip of ``cskip``
        channels], and no group of cout + cskip channels may straddle the concat (320 + 320 does not; 640 + 320 has groups of 30)."""
        if cskip is None or not self.fuse_gn2:
            return False
        cpg = (cout + cskip) // 32
        return cpg > 0 and cout % cpg == 0 and cskip % cpg == 0

    def _resample(self, P, name, mod, x: Act, mode: str, tile: int = 0, cskip: Optional[int] = None) -> Act:
        """cskip (mode 'up'): the channels of the skip map that the next decoder block concatenates behind this Upsample's output
        (None: no such block) - the phase-major form is planned only where that block's GroupNorm reads it (``_phase_map_readable``)."""
        ops = P.step
        B = self._B
        assert x.perm is None, name
        tab = self._table(x.h, x.w, mode)
        ho, wo = tab.ho, tab.wo
        pl = self._planes(P, B * x.h * x.w, x.c)
        pr = x.prod
        if (pr is not None and self.fuse_split and not pr.out_hi and pr.out_f32 == x.t.data_ptr() and
                (pr.n if isinstance(pr, N.WdGemmArgs) else pr.c) == x.c):
            # the producing GEMM writes the planes beside its fp32 output (one launch and one pass over the tensor less)
            pr.out_hi, pr.out_lo = self._hilo(pl)
            pr.out_pl_ld = x.c
        else:
            ops.append((self.lib.wd_split, (x.t.data_ptr(), x.c, B * x.h * x.w, x.c, 0, *self._hilo(pl), x.c), name + ":split"))
        out = self._f32(P, B * ho * wo, mod.cout)
        hw = x.h * x.w
        src4 = None
        if (mode == "up" and tile == 0 and (name + ".wph0") in self._w and self._up_phases_ok(mod) and
                self._phase_map_readable(mod.cout, cskip) and wdirect_fills_chip(B * 4 * hw, mod.cout)):
            # four 2x2 convolutions of the source map, one per output phase: 4 taps instead of 9, the weight image picked per tile;
            # the rows of a sample come out phase-major (Act.perm: the decoder block's GroupNorm reads them in raster order)
            key = (x.h, x.w, "up4")
            if key not in self._tabs:
                t4, pm = upsample_phase_tables(x.h, x.w)
                self._tabs[key] = (GatherTable(torch.from_numpy(t4).to(self.device), ho, wo, t4), torch.from_numpy(pm).to(self.device))
            tab4, perm = self._tabs[key]
            src4 = self._src(pl, x.c, 4, tab4, hw)
            groups = (4, mod.cout * 4 * x.c)
            if not self._wdirect_ok([src4], B * 4 * hw, mod.cout, 4 * hw, w_ngroups=groups[0], w_group_stride=groups[1]):
                src4 = None
        if src4 is not None:
            if (name + ".wph0") not in self._wf:   # the four fragment-major images side by side (one base + a stride for the kernel)
                grp = torch.empty((2, 4, mod.cout, 4 * x.c), dtype=torch.bfloat16, device=self.device)
                st = torch.cuda.current_stream(self.device).cuda_stream
                for ph in range(4):
                    self._wf[f"{name}.wph{ph}"] = grp[:, ph]
                    self._pack_wf(f"{name}.wph{ph}", grp[:, ph], st)
                self._pack = None
            gg = self._gemm(ops, name + ".conv (4 phases)", [src4], name + ".wph0", B * 4 * hw, 4 * hw,
                            bias=self._w[name + ".b"], out_f32=out, out_ld=mod.cout, want_stats=True, w_groups=groups)
            return Act(out, mod.cout, ho, wo, gg.stats, prod=None, perm=perm)
        gg = self._gemm(ops, name + ".conv", [self._src(pl, x.c, 9, tab, x.h * x.w)], name + ".w", B * ho * wo, ho * wo,
                        bias=self._w[name + ".b"], out_f32=out, out_ld=mod.cout, want_stats=True, tile=tile)
        return Act(out, mod.cout, ho, wo, gg.stats, prod=gg.args)

    def _attention(self, ops, what, q, ldq, k, ldk, v, ldv, heads, nq, nk, d, scale, out_pl, out_f32=None,
                   out_rows=None, out_row0=0):
        B = self._B
        ops.append((self.lib.wd_attention,
                    (q, ldq, k, ldk, v, ldv, B, heads, nq, nk, d, float(scale), _ptr(out_f32), *self._hilo(out_pl),
                     out_pl.shape[2] if out_pl is not None else out_f32.shape[-1],
                     nq if out_rows is None else out_rows, out_row0), what))

    def _xattn_fold(self, P, at, heads, d):
        """K/V/to_q/to_out of the cross-attention ``at`` (its ``kv_off`` key) folded per sample in the conditioning phase
        (csrc/wd_xattn.hip): (mq, mo) fp32 and their MFMA operand images (mq_pl, mot_pl)."""
        B, L, inner = self._B, self._ctx_len, heads * d
        ko = self.kv_off[at]
        mq = self._f32(P, B, heads * L, inner)
        mo = self._f32(P, B, heads * L, inner)
        mq_pl = torch.zeros((B, 2, 64, inner), dtype=torch.bfloat16, device=self.device)   # MFMA operands (padded rows 0)
        mot_pl = torch.zeros((B, 2, inner, 64), dtype=torch.bfloat16, device=self.device)
        P.keep += [mq_pl, mot_pl]
        P.cond.append((self.lib.wd_xattn_fold,
                       (self._kv.data_ptr() + 4 * ko, self.kv_total, self._kv.data_ptr() + 4 * (ko + inner), self.kv_total, B,
                        heads, L, d, float(d ** -0.5), self._w[at + ".q.f32"].data_ptr(), self._w[at + ".o.f32"].data_ptr(), inner,
                        mq.data_ptr(), mo.data_ptr(), mq_pl.data_ptr(), mot_pl.data_ptr()), at + ":fold"))
        return mq, mo, mq_pl, mot_pl

    def _xattn_mfma(self) -> bool:
        """Do the folded cross-attention launches run on the MFMA units?  WDIFF_XATTN_VALU selects their fp32 VALU form, which writes
        no operand planes of its result and is not the arithmetic wd_xattn_maps repeats.  Read at plan time, not in __init__: the C
        side reads the variable at every call."""
        return not os.environ.get("WDIFF_XATTN_VALU")

    def _ff_fills_chip(self, p, M) -> bool:
        """Does block ``p`` run its feed-forward as wd_ff_fused?  One workgroup per 64 tokens: worth it once they fill the chip (the
        8 x 32 level at batch >= 48)."""
        return self.fuse_ff and (p + ".ff1f.w") in self._w and (M + 63) // 64 >= 192

    def _st_form(self, P, name, mod: SpatialTransformerParams, x: Act) -> StForm:
        """The launch form of SpatialTransformer ``name`` reading the map ``x`` under this engine's switches, with the sizes every
        stage needs (DESIGN.md "SpatialTransformer launch forms" is this function as a table)."""
        B, h, w, c = self._B, x.h, x.w, x.c
        hw, M = h * w, B * h * w
        heads, d, L = mod.heads, mod.d_head, self._ctx_len
        inner = heads * d
        nblk = len(mod.transformer_blocks)
        tap = name in P.map_taps
        xfold = self.fuse_xattn and bool(self.lib.wd_xattn_supported(inner, heads, L))  # K/V/to_q/to_out folded per sample (<= 10 keys)
        # asked once, before anything of the block is planned: where ``x`` has no statistics yet the question appends their
        # wd_gn_stats launch, which is the block's first op in every form
        gn_in = self._gn_in_consumer(P, P.step, name + ".gn", [x], False, M, hw, inner)
        one_launch = (
            self.fuse_st and                          # WDIFF_FUSE_ST=0: the tests' reference for this form
            not tap and                               # its attn2 softmax is read back (attention maps): needs attn2's input in memory
            self.variant != "phosc" and               # the front runs two cross-attentions; PHOSC blocks start with self-attention
            nblk == 1 and                             # the front feeds the feed-forward and proj_out tail of the same block
            inner == c == 320 and                     # the kernel is built for 320-channel rows
            self.npass == 3 and                       # ... and for split-bf16 operands
            xfold and self.fuse_xattn_pair and        # it is the pair form kept on chip: each switch that undoes that undoes this
            self.fuse_ff and self.fuse_proj and       # the front only comes with the feed-forward + proj_out tail
            (M + 63) // 64 >= 192 and                 # one workgroup per 64-token panel: they must fill the chip
            hw % 64 == 0 and                          # a panel must not straddle two samples
            (name + ".tb0.ff1f.w") in self._w and     # wd_ff_supported(inner, hidden width): the weights were packed for it
            gn_in)                                    # the front normalises the fp32 map as proj_in's own staging would
        if one_launch:
            form = "one-launch"
        elif xfold and self.variant != "phosc" and self.fuse_xattn_pair:
            form = "pair"
        elif self.variant == "phosc":
            form = "phosc"
        else:
            form = "folded" if xfold else "plain"
        ff_fused = self._ff_fills_chip(f"{name}.tb{nblk - 1}", M)
        if ff_fused and self.fuse_proj and inner == c:
            tail = "ff+proj"
        elif (not ff_fused and self.fold_proj and self.npass == 3 and (name + ".po32.w") in self._w and
              xfold and self._xattn_mfma()):   # (tok2 as operand planes: the MFMA form of the folded cross-attention writes them)
            tail = "two-source"
        else:
            tail = "proj_out"
        return StForm(form, tail, B, h, w, c, hw, M, heads, d, inner, L, tap, gn_in, xfold)

    def _transformer(self, P, name, mod: SpatialTransformerParams, x: Act) -> Act:
        f = self._st_form(P, name, mod, x)
        if f.form == "one-launch":
            return self._transformer_fused(P, f, name, mod, x)
        return self._transformer_chain(P, f, name, mod, x)

    def _transformer_chain(self, P, f: StForm, name, mod: SpatialTransformerParams, x: Act) -> Act:
        """proj_in, then per block the attentions of ``f.form`` and the feed-forward; the last block ends in the tail ``f.tail``."""
        tok, n1 = self._st_proj_in(P, f, name, x)
        for di, tb in enumerate(mod.transformer_blocks):
            p = f"{name}.tb{di}"
            last = di == len(mod.transformer_blocks) - 1
            ffi = tb.ff.net[2].in_features
            tok2pl = self._planes(P, f.M, f.inner) if last and f.tail == "two-source" else None
            tok2, n3, tapped = self._st_attention(P, f, p, tok, n1 if di == 0 else None, tok2pl)
            if f.tap:
                self._st_maps(P, f, p, *tapped)
            if n3 is None:
                n3 = self._ln(P, P.step, p + ".norm3", tok2, f.M, f.inner, p + ".norm3")
            if last:
                return self._st_tail(P, f, name, p, ffi, n3, tok2, tok2pl, x)
            tok = self._f32(P, f.M, f.inner)
            self._st_ff(P, f, p, ffi, n3, tok2, tok, None)

    def _st_proj_in(self, P, f: StForm, name, x: Act):
        """GroupNorm + proj_in -> the token rows [M, inner]; f.gn_in: the GEMM normalises the fp32 map itself while it stages it.
        Also returns the first block's norm1 planes where proj_in's epilogue wrote them (PHOSC variant, tiles that hold whole rows)."""
        tok = self._f32(P, f.M, f.inner)
        if f.gn_in:
            src, a32 = self._src32(x, hw_src=f.hw), (x, name + ".gn", 1e-6, False)
        else:
            g, _ = self._gn(P, P.step, name + ".gn", [x], name + ".gn", 1e-6, False)
            src, a32 = self._src(g, f.c), None
        g_in = self._gemm(P.step, name + ".proj_in", [src], name + ".pi.w", f.M, f.hw, bias=self._w[name + ".pi.b"], out_f32=tok,
                          out_ld=f.inner, a32=a32, ln=f"{name}.tb0.norm1" if self.variant == "phosc" else None)
        return tok, g_in.ln_pl

    def _st_attention(self, P, f: StForm, p, tok, n1, tok2pl):
        """attn1 and attn2 of block ``p`` as ``f.form`` plans them -> (tok2, norm3 planes or None, what a maps tap reads).
        n1: norm1 planes already made (PHOSC).  tok2pl: planes that also take tok2 itself."""
        if f.form == "pair":
            return self._st_attn_pair(P, f, p, tok, tok2pl)
        n2 = None
        if f.form == "phosc":
            tok1, n2 = self._st_attn_self(P, f, p, tok, n1)
        elif f.form == "folded":
            tok1, _, _ = self._st_attn_folded(P, f, p, "a1", tok)
        else:  # (the base model reads norm2 for both attentions, unet.py:337-345)
            tok1, _ = self._st_attn_plain(P, f, p, "a1", tok, self._ln(P, P.step, p + ".norm2a", tok, f.M, f.inner, p + ".norm2"))
        if f.xfold:
            tok2, n3, fold = self._st_attn_folded(P, f, p, "a2", tok1, next_ln="norm3", raw=tok2pl)
            return tok2, n3, (tok1, None, fold)
        if n2 is None:
            n2 = self._ln(P, P.step, p + ".norm2", tok1, f.M, f.inner, p + ".norm2")
        return (*self._st_attn_plain(P, f, p, "a2", tok1, n2, next_ln="norm3", pack=self.pack_kv), None)

    def _st_attn_pair(self, P, f: StForm, p, x_in, raw=None):
        """Both cross-attentions of a base-model block (each behind norm2, unet.py:337-345) and norm3 in one launch.  raw: planes
        that take the result itself (wd_xattn_planes)."""
        w, inner = self._w, f.inner
        fa, fb = (self._xattn_fold(P, f"{p}.{tag}", f.heads, f.d)[2:] for tag in ("a1", "a2"))
        x_out, npl = self._f32(P, f.M, inner), self._planes(P, f.M, inner)
        g2, b2 = w[f"{p}.norm2.g"].data_ptr(), w[f"{p}.norm2.b"].data_ptr()
        args = (x_in.data_ptr(), inner, f.B, f.hw, inner, 1e-5, f.heads, f.L, g2, b2, fa[0].data_ptr(), fa[1].data_ptr(),
                w[f"{p}.a1.o.b"].data_ptr(), g2, b2, fb[0].data_ptr(), fb[1].data_ptr(), w[f"{p}.a2.o.b"].data_ptr(),
                x_out.data_ptr(), inner, w[f"{p}.norm3.g"].data_ptr(), w[f"{p}.norm3.b"].data_ptr(), 1e-5, *self._hilo(npl), inner)
        if raw is not None:
            P.step.append((self.lib.wd_xattn_planes, args + (*self._hilo(raw), inner), f"{p}.a1+a2:folded + planes"))
        else:
            P.step.append((self.lib.wd_xattn_pair, args, f"{p}.a1+a2:folded"))
        return x_out, npl, (x_in, fa, fb)

    def _st_attn_folded(self, P, f: StForm, p, tag, x_in, next_ln=None, raw=None):
        """x_out = x_in + to_out(attention(to_q(norm2(x_in)), K, V)) in one launch.  next_ln: also emit the following LayerNorm as
        operand planes.  raw: planes that take x_out itself (wd_xattn_planes).  Returns (x_out, those LayerNorm planes, the fold)."""
        w, inner = self._w, f.inner
        mq, mo, mq_pl, mot_pl = self._xattn_fold(P, f"{p}.{tag}", f.heads, f.d)
        x_out = self._f32(P, f.M, inner)
        npl = self._planes(P, f.M, inner) if next_ln else None
        src = (x_in.data_ptr(), inner, f.B, f.hw, inner)
        ln = (w[f"{p}.norm2.g"].data_ptr(), w[f"{p}.norm2.b"].data_ptr())
        bias = w[f"{p}.{tag}.o.b"].data_ptr()
        dst = (x_out.data_ptr(), inner, w[f"{p}.{next_ln}.g"].data_ptr() if next_ln else None,
               w[f"{p}.{next_ln}.b"].data_ptr() if next_ln else None, 1e-5, *self._hilo(npl), inner)
        if raw is not None:  # (the pair entry point with no second attention)
            P.step.append((self.lib.wd_xattn_planes,
                           (*src, 1e-5, f.heads, f.L, *ln, mq_pl.data_ptr(), mot_pl.data_ptr(), bias, None, None, None, None, None,
                            *dst, *self._hilo(raw), inner), f"{p}.{tag}:folded + planes"))
        else:
            P.step.append((self.lib.wd_xattn_fused,
                           (*src, *ln, 1e-5, mq.data_ptr(), mo.data_ptr(), f.heads, f.L, bias, *dst, mq_pl.data_ptr(),
                            mot_pl.data_ptr()), f"{p}.{tag}:folded"))
        return x_out, npl, (mq_pl, mot_pl)

    def _st_attn_self(self, P, f: StForm, p, tok, n1):
        """attn1 of a PHOSC block: self-attention over the hw tokens of a sample as wd_gemm (q, k, v) -> wd_attention -> wd_gemm.
        Returns (tok1, norm2 planes or None): the planes come out of the last epilogue where a plain attn2 would read them."""
        ops, M, hw, inner = P.step, f.M, f.hw, f.inner
        if n1 is None:
            n1 = self._ln(P, ops, p + ".norm1", tok, M, inner, p + ".norm1")
        qkv = self._f32(P, M, 3 * inner)
        self._gemm(ops, p + ".a1.qkv", [self._src(n1, inner)], p + ".a1.qkv.w", M, hw, out_f32=qkv, out_ld=3 * inner)
        o1 = self._planes(P, M, inner)
        self._attention(ops, p + ".a1", qkv.data_ptr(), 3 * inner, qkv.data_ptr() + 4 * inner, 3 * inner,
                        qkv.data_ptr() + 8 * inner, 3 * inner, f.heads, hw, hw, f.d, f.d ** -0.5, o1)
        tok1 = self._f32(P, M, inner)
        g = self._gemm(ops, p + ".a1.out", [self._src(o1, inner)], p + ".a1.o.w", M, hw, bias=self._w[p + ".a1.o.b"],
                       resid=tok.data_ptr(), resid_ld=inner, out_f32=tok1, out_ld=inner, ln=None if f.xfold else p + ".norm2")
        return tok1, g.ln_pl

    def _st_attn_plain(self, P, f: StForm, p, tag, x_in, n_in, next_ln=None, pack=False):
        """x_out = x_in + to_out(attention(to_q(n_in), K, V)) over the context's keys as wd_gemm -> wd_attention -> wd_gemm.  n_in:
        the LayerNorm planes of x_in.  next_ln: the last epilogue also writes that LayerNorm of x_out where it can.  pack: a long
        context's keys / values as LDS images.  Returns (x_out, the next_ln planes or None)."""
        ops, M, hw, inner, heads, L, d = P.step, f.M, f.hw, f.inner, f.heads, f.L, f.d
        q = self._f32(P, M, inner)
        self._gemm(ops, f"{p}.{tag}.q", [self._src(n_in, inner)], f"{p}.{tag}.q.w", M, hw, out_f32=q, out_ld=inner)
        ko = self.kv_off[f"{p}.{tag}"]
        o = self._planes(P, M, inner)
        kp, vp = self._kv.data_ptr() + 4 * ko, self._kv.data_ptr() + 4 * (ko + inner)
        nimg = self.lib.wd_attention_packed_elems(f.B, heads, L, d) if pack else 0
        if nimg > 0:
            # the context's keys / values do not change during a sampling call: their split-bf16 LDS images are built
            # once per call (P.cond, after the K/V projection) and every step's attention copies them 16 bytes at a time
            img = torch.empty(nimg, dtype=torch.bfloat16, device=self.device)
            P.keep.append(img)
            P.cond.append((self.lib.wd_attention_pack_kv,
                           (kp, self.kv_total, vp, self.kv_total, f.B, heads, L, d, img.data_ptr()), f"{p}.{tag}:pack kv"))
            ops.append((self.lib.wd_attention_packed,
                        (q.data_ptr(), inner, img.data_ptr(), f.B, heads, hw, L, d, float(d ** -0.5), None, *self._hilo(o), inner,
                         hw, 0), f"{p}.{tag}"))
        else:
            self._attention(ops, f"{p}.{tag}", q.data_ptr(), inner, kp, self.kv_total, vp, self.kv_total, heads, hw, L, d,
                            d ** -0.5, o)
        x_out = self._f32(P, M, inner)
        g = self._gemm(ops, f"{p}.{tag}.out", [self._src(o, inner)], f"{p}.{tag}.o.w", M, hw, bias=self._w[f"{p}.{tag}.o.b"],
                       resid=x_in.data_ptr(), resid_ld=inner, out_f32=x_out, out_ld=inner, ln=f"{p}.{next_ln}" if next_ln else None)
        return x_out, g.ln_pl

    def _st_maps(self, P, f: StForm, p, x_in, fa, fb):
        """The attn2 softmax of block ``p`` summed over heads into this tap's map buffer.  x_in is what the attention launch just
        before read: the rows attn1 reads (fa: attn1's fold - the pair form runs attn1 again) or attn2's own input (fa None)."""
        w = self._w
        g2, b2 = w[f"{p}.norm2.g"].data_ptr(), w[f"{p}.norm2.b"].data_ptr()
        first = (g2, b2, fa[0].data_ptr(), fa[1].data_ptr(), w[f"{p}.a1.o.b"].data_ptr()) if fa is not None else (None,) * 5
        buf = torch.zeros((f.B, f.hw, f.L), dtype=torch.float32, device=self.device)
        P.maps.append(buf)
        P.map_hw.append((f.h, f.w))
        wt = P.map_w
        P.step.append((self.lib.wd_xattn_maps,
                       (x_in.data_ptr(), f.inner, f.B, f.hw, f.inner, 1e-5, f.heads, f.L, *first, g2, b2, fb[0].data_ptr(),
                        buf.data_ptr(), f.L, _ptr(wt), wt.numel() if wt is not None else 0,
                        P.map_k.data_ptr() if wt is not None else None), f"{p}.a2:maps"))

    def _st_ff1(self, P, f: StForm, p, ffi, n3):
        """The GEGLU projection of block ``p`` as a GEMM -> the hidden activations as operand planes [M, ffi]."""
        ffh = self._planes(P, f.M, ffi)
        self._gemm(P.step, p + ".ff1", [self._src(n3, f.inner)], p + ".ff1.w", f.M, f.hw, bias=self._w[p + ".ff1.b"],
                   act=N.ACT_GEGLU, out_pl=ffh, tile=geglu_tile(ffi))
        return ffh

    def _st_ff(self, P, f: StForm, p, ffi, n3, tok2, out_f32, out_pl):
        """tok2 + FeedForward(n3) into fp32 rows and / or operand planes: one wd_ff_fused launch where that fills the chip, else the
        GEGLU GEMM and ff2."""
        if self._ff_fills_chip(p, f.M):
            self._ff_fused(P.step, p, n3, tok2, f.M, f.inner, ffi, out_f32, out_pl)
            return
        ffh = self._st_ff1(P, f, p, ffi, n3)
        self._gemm(P.step, p + ".ff2", [self._src(ffh, ffi)], p + ".ff2.w", f.M, f.hw, bias=self._w[p + ".ff2.b"],
                   resid=tok2.data_ptr(), resid_ld=f.inner, out_f32=out_f32, out_ld=f.inner, out_pl=out_pl)

    def _st_tail(self, P, f: StForm, name, p, ffi, n3, tok2, tok2pl, x: Act) -> Act:
        """The last block's feed-forward, proj_out and the transformer's residual as ``f.tail`` plans them -> the output map, with
        the statistics of the next ResBlock's GroupNorm where the last launch gives them."""
        ops, M, hw, c = P.step, f.M, f.hw, f.c
        out = self._f32(P, M, c)
        if f.tail == "ff+proj":
            g = self._ff_fused(ops, p, n3, tok2, M, f.inner, ffi, out, None, proj=(name, x.t, hw))
        elif f.tail == "two-source":  # ff2 and proj_out folded: out = [h | tok2] [W32 | W3]^T + b32 + x
            ffh = self._st_ff1(P, f, p, ffi, n3)
            g = self._gemm(ops, name + ".ff2 + proj_out", [self._src(ffh, ffi), self._src(tok2pl, f.inner)], name + ".po32.w", M, hw,
                           bias=self._w[name + ".b32"], resid=x.t.data_ptr(), resid_ld=c, out_f32=out, out_ld=c, want_stats=True)
        else:
            xpl = self._planes(P, M, f.inner)
            self._st_ff(P, f, p, ffi, n3, tok2, None, xpl)
            g = self._gemm(ops, name + ".proj_out", [self._src(xpl, f.inner)], name + ".po.w", M, hw, bias=self._w[name + ".po.b"],
                           resid=x.t.data_ptr(), resid_ld=c, out_f32=out, out_ld=c, want_stats=True)
        return Act(out, c, f.h, f.w, g.stats, prod=g.args)

    def _transformer_fused(self, P, f: StForm, name, mod: SpatialTransformerParams, x: Act) -> Act:
        """The SpatialTransformer (unet.py:398-412, one base-model block) as ONE wd_ff_fused launch with the transformer front
        (wd_ff_args.x_in): GroupNorm + proj_in, both folded cross-attentions, norm3, the GEGLU feed-forward and proj_out + residual
        per 64-token panel; the GroupNorm statistics of the result for the next ResBlock come out of its epilogue."""
        M, hw, c, heads, d, L = f.M, f.hw, f.c, f.heads, f.d, f.L
        p = name + ".tb0"
        folds = [self._xattn_fold(P, f"{p}.{tag}", heads, d)[2:] for tag in ("a1", "a2")]
        # (folded tail: the kernel keeps tok2 on chip - no scratch)
        tok2 = None if self._fold_fused(name) else self._f32(P, M, c)
        out = self._f32(P, M, c)
        part, nchunk, pc = x.stats
        pw = self._wfrag(name + ".pi.w")
        front = dict(x_in=x.t.data_ptr(), x_in_ld=c, hw=hw, gn_part=part.data_ptr(), gn_nchunk=nchunk, gn_pcpg=pc, gn_cpg=c // 32,
                     gn_eps=1e-6, gn_gamma=self._w[name + ".gn.g"].data_ptr(), gn_beta=self._w[name + ".gn.b"].data_ptr(),
                     pi_hi=pw[0].data_ptr(), pi_lo=pw[1].data_ptr(), pi_b=self._w[name + ".pi.b"].data_ptr(),
                     ln2_gamma=self._w[p + ".norm2.g"].data_ptr(), ln2_beta=self._w[p + ".norm2.b"].data_ptr(),
                     mq_a=folds[0][0].data_ptr(), mot_a=folds[0][1].data_ptr(), xb_a=self._w[p + ".a1.o.b"].data_ptr(),
                     mq_b=folds[1][0].data_ptr(), mot_b=folds[1][1].data_ptr(), xb_b=self._w[p + ".a2.o.b"].data_ptr(),
                     ln3_gamma=self._w[p + ".norm3.g"].data_ptr(), ln3_beta=self._w[p + ".norm3.b"].data_ptr(), ln_eps=1e-5,
                     heads=heads, L=L, tok2=_ptr(tok2))
        ffi = mod.transformer_blocks[0].ff.net[2].in_features
        fa = self._ff_fused(P.step, p, None, tok2, M, c, ffi, out, None, proj=(name, x.t, hw), front=front)
        return Act(out, c, x.h, x.w, fa.stats, prod=fa.args)

    def _fold_fused(self, name) -> bool:
        """Does wd_ff_fused run the proj_out tail of SpatialTransformer ``name`` folded (wd_ff_args.w32_*)?"""
        return self.fold_proj and self.npass == 3 and (name + ".w32.w") in self._w

    def _wfrag(self, wname):
        """The fragment-major image (wd_gemm_pack_w) of a packed matrix, kept up to date by refresh_weights."""
        if wname not in self._wf:
            self._wf[wname] = torch.empty_like(self._w[wname])
            self._pack_wf(wname, self._wf[wname], torch.cuda.current_stream(self.device).cuda_stream)
            self._pack = None  # the next refresh_weights rebuilds the repack table with this image in it
        return self._wf[wname]

    def _ff_fused(self, ops, p, n3, resid, M, inner, ffi, out_f32, out_pl, proj=None, front=None):
        """x + FeedForward(LN3(x)) (unet.py:343-344, :122-149) as one wd_ff_fused launch.  proj = (SpatialTransformer name, residual
        tensor, hw): that transformer's proj_out + residual (unet.py:406-412) in the same launch, with the GroupNorm statistics
        of the result for the next ResBlock; returns the statistics tuple then.  front: the wd_ff_args fields of the transformer
        front (n3 is None then: the launch makes the norm3 rows itself)."""
        a = N.WdFfArgs()
        if front is None:
            (a.x_hi, a.x_lo), a.x_ld = self._hilo(n3), n3.shape[2]
        else:
            for k, v in front.items():
                setattr(a, k, v)
        a.m, a.c, a.inner = M, inner, ffi
        w1, w2 = self._wfrag(p + ".ff1f.w"), self._wfrag(p + ".ff2.w")
        a.w1_hi, a.w1_lo, a.b1 = w1[0].data_ptr(), w1[1].data_ptr(), self._w[p + ".ff1f.b"].data_ptr()
        a.w2_hi, a.w2_lo, a.b2 = w2[0].data_ptr(), w2[1].data_ptr(), self._w[p + ".ff2.b"].data_ptr()
        a.resid, a.resid_ld = _ptr(resid), inner
        if out_f32 is not None:
            a.out_f32, a.out_ld = out_f32.data_ptr(), inner
        if out_pl is not None:
            (a.out_hi, a.out_lo), a.out_pl_ld = self._hilo(out_pl), out_pl.shape[2]
        a.hw_out, a.npass = 1, self.npass
        stats = None
        if proj is not None:
            name, x_in, hw = proj
            w3 = self._wfrag(name + ".po.w")
            a.w3_hi, a.w3_lo, a.b3 = w3[0].data_ptr(), w3[1].data_ptr(), self._w[name + ".po.b"].data_ptr()
            a.resid3, a.resid3_ld = x_in.data_ptr(), inner
            if self._fold_fused(name):
                w32 = self._wfrag(name + ".w32.w")
                a.w32_hi, a.w32_lo, a.b32 = w32[0].data_ptr(), w32[1].data_ptr(), self._w[name + ".b32"].data_ptr()
            if self.fuse_stats and inner % 32 == 0 and hw % 64 == 0:
                nchunk = hw // 64
                part = torch.zeros((M // hw, nchunk, 32, 2), dtype=torch.float64, device=self.device)
                self._cur_plan.keep.append(part)
                a.stat_part, a.stat_cpg, a.hw_out = part.data_ptr(), inner // 32, hw
                stats = (part, nchunk, inner // 32)
        if self.epi_batch is not None:
            a.dbg |= N.EPI_BATCH_ON if self.epi_batch else N.EPI_BATCH_OFF
        self._cur_plan.keep.append(a)
        what = ".ff (fused)" if proj is None else ".ff + proj_out (fused)" if front is None else ": gn + proj_in + a1 + a2 + ff + proj_out (fused)"
        ops.append((self.lib.wd_ff_fused, (C.byref(a),), p + what))
        return GemmOp(a, stats)

    # ------------------------------------------------------------------------------------------ plan
    @staticmethod
    def _cached_plan(plans: Dict[tuple, Plan], key, room: int = 0) -> Optional[Plan]:
        """The plan kept under ``key`` (now the most recently used one), or None; then, for an engine that keeps at most
        ``room`` plans, the least recently used ones go before the caller builds its own (a plan holds ~1 GB of buffers at
        B = 64).  The caller stores what it built as ``plans[key]``."""
        if key in plans:
            plans[key] = plans.pop(key)  # most recently used last
            return plans[key]
        while room and len(plans) >= room:
            plans.pop(next(iter(plans)))
        return None

    def _begin_plan(self, P: Plan, B: int) -> Plan:
        """Every block builder (_gemm, _gn, _resblock, ...) reads the plan under construction and its batch from the engine."""
        self._cur_plan = P
        self._B = B
        return P

    def _inputs(self, P: Plan, H, W, ctx_len, phosc_len):
        """Persistent inputs (the caller copies into these, ``load_inputs``; graph replays read them).  An absent token group
        keeps one column, so that the buffer has an address."""
        m, B, dev = self.model, self._B, self.device
        P.x_in = torch.zeros((B, m.in_channels, H, W), dtype=torch.float32, device=dev)
        P.t_in = torch.zeros((B,), dtype=torch.int64, device=dev)
        P.y_in = torch.zeros((B,), dtype=torch.int64, device=dev)
        P.ctx_in = torch.zeros((B, max(ctx_len, 1)), dtype=torch.int64, device=dev)
        P.phosc_in = torch.zeros((B, max(phosc_len, 1)), dtype=torch.int32, device=dev)

    def _conditioning(self, P: Plan, ops, ctx_len, phosc_len) -> List[tuple]:
        """CharacterEncoder (unet.py:851-874) of each token group into ``P.ctx_pl`` + K/V of every cross-attention (``self._kv``).
        Returns (ids, n_tok, row0, i64, embedding planes, qkv) per group: what a backward pass through it reads."""
        m, lib, B = self.model, self.lib, self._B
        cd = m.context_dim
        msl = m.max_seq_len
        L = self._ctx_len = ctx_len + phosc_len
        P.ctx_pl = self._planes(P, B * L, cd)
        groups = []
        for (ids, n_tok, row0, i64) in ((P.ctx_in, ctx_len, 0, 1), (P.phosc_in, phosc_len, ctx_len, 0)):
            if n_tok == 0:
                continue
            use_pe = (self.variant == "base") or (n_tok <= msl)  # unetPhosc.py:726-729 skips the table for PHOSC vectors
            if use_pe and n_tok > msl:
                raise ValueError(f"context length {n_tok} exceeds max_seq_len {msl} (the reference fails too)")
            e = self._planes(P, B * n_tok, cd)
            ops.append((lib.wd_embed_tokens,
                        (ids.data_ptr(), i64, B * n_tok, n_tok, self._w["we.table"].data_ptr(), self._w["we.table"].shape[0], cd,
                         self._w["pe"].data_ptr() if use_pe else None, *self._hilo(e), cd), "word_emb.embedding"))
            qkv = self._f32(P, B * n_tok, 3 * cd)
            self._gemm(ops, "word_emb.qkv", [self._src(e, cd)], "we.qkv.w", B * n_tok, n_tok, bias=self._w["we.qkv.b"],
                       out_f32=qkv, out_ld=3 * cd)
            # Word_Attention: softmax(q k^T) v without 1/sqrt(d) (unet.py:831-835)
            self._attention(ops, "word_emb.attention", qkv.data_ptr(), 3 * cd, qkv.data_ptr() + 4 * cd, 3 * cd,
                            qkv.data_ptr() + 8 * cd, 3 * cd, 1, n_tok, n_tok, cd, 1.0, P.ctx_pl, out_rows=L, out_row0=row0)
            groups.append((ids, n_tok, row0, i64, e, qkv))
        if self.kv_total:
            self._kv = self._f32(P, B * L, self.kv_total)
            self._gemm(ops, "cross.kv", [self._src(P.ctx_pl, cd)], "kv.w", B * L, L, out_f32=self._kv, out_ld=self.kv_total)
        return groups

    def _head_gemm(self, P: Plan, ops, what, x: torch.Tensor, w: str, label="im2col", want_stats=True, tile=0):
        """3x3 / pad 1 convolution ``w`` (weights ``w``.w over the padded im2col width ``kpad_in``, bias ``w``.b) of an NCHW fp32
        tensor with few channels: wd_im2col3x3 into operand planes + one GEMM.  Returns the token-major result (with its
        GroupNorm statistics where wanted and available) and the im2col planes."""
        B, cin, H, W = x.shape
        xin = self._planes(P, B * H * W, self.kpad_in)
        ops.append((self.lib.wd_im2col3x3, (x.data_ptr(), B, cin, H, W, *self._hilo(xin), self.kpad_in), label))
        cout = self._w[w + ".w"].shape[1]
        h0 = self._f32(P, B * H * W, cout)
        g0 = self._gemm(ops, what, [self._src(xin, self.kpad_in)], w + ".w", B * H * W, H * W, bias=self._w[w + ".b"], out_f32=h0,
                        out_ld=cout, want_stats=want_stats, tile=tile)
        return Act(h0, cout, H, W, g0.stats), xin

    def _map_taps(self, L: int) -> tuple:
        """The three SpatialTransformers whose attn2 softmax the reference returns with --attentionMaps 1 (unet.py:1645-1832: the
        last one of the input blocks, the middle one, the last one of the output blocks), by the names ``_trunk`` gives them.
        Raises NotImplementedError where one of them does not run on the folded MFMA cross-attention - the only form whose
        probabilities ``wd_xattn_maps`` reproduces."""
        m = self.model
        if self.variant == "phosc":
            raise NotImplementedError("attention maps: the PHOSC model's cross-attention has ctx + PHOSC keys, and the reference "
                                      "keeps a map only where it has 10 (unetPhosc.py: attn.shape[-1] == 10 is false)")
        if not self.fuse_xattn or not self._xattn_mfma():
            raise NotImplementedError("attention maps need the folded MFMA cross-attention (WDIFF_FUSE_XATTN=0 / WDIFF_XATTN_VALU "
                                      "select forms that do not keep the probabilities wd_xattn_maps reports)")
        taps = []
        for prefix, blocks in (("in", list(enumerate(m.input_blocks))[1:]), ("mid", [(None, m.middle_block)]),
                               ("out", list(enumerate(m.output_blocks)))):
            found = [(f"{prefix}{'' if i is None else i}.{j}", mod) for i, blk in blocks for j, mod in enumerate(blk)
                     if isinstance(mod, SpatialTransformerParams)]
            if not found:
                raise NotImplementedError(f"attention maps: no SpatialTransformer in the {prefix} blocks")
            name, mod = found[-1]
            if len(mod.transformer_blocks) != 1:
                raise NotImplementedError("attention maps with transformer_depth > 1 (the reference keeps the last block's map; "
                                          "not planned here)")
            if not self.lib.wd_xattn_supported(mod.heads * mod.d_head, mod.heads, L):
                raise NotImplementedError(f"attention maps: {name} ({mod.heads * mod.d_head} channels, {mod.heads} heads, {L} "
                                          "keys) is outside wd_xattn_supported")
            taps.append(name)
        return tuple(taps)

    def _trunk(self, P: Plan, cur: Act) -> Act:
        """Input blocks after the first convolution, middle block, output blocks over the skip stack."""
        m = self.model
        hs = [cur]

        def run_layers(prefix, blk, cur, extra=None, cskip=None):
            """extra: the skip map the block's first ResBlock concatenates; cskip: the channels of the skip map the NEXT block will."""
            for j, mod in enumerate(blk):
                name = f"{prefix}.{j}"
                if isinstance(mod, ResBlockParams):
                    cur = self._resblock(P, name, mod, [cur] + ([extra] if (extra is not None and j == 0) else []))
                elif isinstance(mod, SpatialTransformerParams):
                    cur = self._transformer(P, name, mod, cur)
                elif isinstance(mod, DownsampleParams):
                    cur = self._resample(P, name, mod, cur, "down")
                elif isinstance(mod, UpsampleParams):
                    cur = self._resample(P, name, mod, cur, "up", cskip=cskip if j == len(blk) - 1 else None)
                else:
                    raise TypeError(type(mod))
            return cur

        for i, blk in enumerate(m.input_blocks):
            if i == 0:
                continue
            cur = run_layers(f"in{i}", blk, cur)
            hs.append(cur)
        cur = run_layers("mid", m.middle_block, cur)
        for i, blk in enumerate(m.output_blocks):
            extra = hs.pop()
            cur = run_layers(f"out{i}", blk, cur, extra=extra, cskip=hs[-1].c if hs else None)
        return cur

    def _tail_gemm(self, P: Plan, ops, what, x: Act, eps, nchw: Optional[torch.Tensor] = None):
        """GroupNorm ``out.gn`` + SiLU into operand planes, then the 3x3 / pad 1 convolution ``out.w`` as a GEMM into token rows;
        ``nchw``: the tensor a wd_tokens_to_nchw launch then writes them to.  Returns the planes and the token rows."""
        B, hw = self._B, x.h * x.w
        g, _ = self._gn(P, ops, "out.gn", [x], "out.gn", eps, True)
        tab = self._table(x.h, x.w, "same")
        oc = self._w["out.w"].shape[1]
        otok = self._f32(P, B * hw, oc)
        self._gemm(ops, what, [self._src(g, x.c, 9, tab, hw)], "out.w", B * hw, hw, bias=self._w["out.b"], out_f32=otok, out_ld=oc)
        if nchw is not None:
            ops.append((self.lib.wd_tokens_to_nchw, (otok.data_ptr(), oc, B, oc, hw, nchw.data_ptr()), "tokens_to_nchw"))
        return g, otok

    def plan(self, B: int, H: int, W: int, ctx_len: int, phosc_len: int, film_steps: int = 0, mix: int = 0,
             film_timesteps: Optional[tuple] = None, attn_maps: bool = False, attn_rows: int = 0,
             attn_by_step: bool = False, guide: int = 0, writer_keep: bool = False) -> Plan:
        """film_steps = T > 0 (the DDPM sampler): the whole time / writer embedding path (timestep_embedding, time_embed,
        label_emb, SiLU, every emb_layers) is tabulated for all T timesteps by ``P.film`` ops - one large GEMM per
        ``sampling()`` call instead of three 64-row GEMMs per step - and each step copies its rows (``wd_select_rows``).

        mix > 0 (writer-style interpolation, unet.py:1558-1573): the label term of a sample is the blend of a pair of writers
        (``P.pairs`` / ``P.mix_m``, filled by ``load_mix``) instead of ``label[y]``.  With the table, ``mix`` is the number of
        forwards per step (1 or 2) that read rows of their own - pairs indexed (forward, t, b); ``P.step`` reads the rows of
        forward 0 and writes ``P.out``, ``P.step1`` (mix = 2) those of forward 1 and writes ``P.out1``.

        film_timesteps = tau (the DDIM sampler, with film_steps = T): the table covers the S visited timesteps only - row k is
        timestep tau[k], ``P.film_prepare`` takes the step index k, ``wd_select_rows`` reads it from ``P.k_dev`` and the pairs
        of the interpolation path are indexed (forward, k, b).

        attn_maps: the three tapped SpatialTransformers (``_map_taps``) run as the chained launches (never the one-launch form)
        and each gains one ``wd_xattn_maps`` launch after its attention launch, into ``P.maps[i]`` fp32 [B, h_i*w_i, L].  Every
        other launch is the default plan's with WDIFF_FUSE_ST=0 for those three blocks.  attn_rows = 0: a step overwrites the
        maps.  attn_rows = R > 0 (the samplers): a step adds ``P.map_w[row] * map``, ``P.map_w`` fp32 [R] filled by the caller,
        row = ``P.k_dev`` if attn_by_step else ``P.t_dev``; with mix = 2 only the first forward of a step adds.

        guide = 2 (writer-free guidance, with the table): a two-forward plan built as mix = 2 is - ``P.step`` reads the rows of
        forward 0, SiLU(time + label[y]), ``P.step1`` those of forward 1, SiLU(time) (``wd_emb_combine_keep`` without a keep
        mask), and writes ``P.out1``.  Not together with mix.
        writer_keep (without the table): the writer term per sample - ``wd_label_rows_keep`` turns ``P.keep_in`` (uint8 [B],
        filled by ``load_keep``) into the residual rows of the time_embed.2 GEMM, label[y_b] or zeros."""
        key = (B, H, W, ctx_len, phosc_len, self.npass, film_steps) + ((("mix", mix),) if mix else ())
        if guide:
            key += (("guide", guide),)
        if writer_keep:
            key += (("writer_keep",),)
        if attn_maps:
            key += (("maps", int(attn_rows), bool(attn_by_step)),)
        if film_timesteps is not None:
            film_timesteps = tuple(int(t) for t in film_timesteps)
            if not film_steps or not film_timesteps or min(film_timesteps) < 0 or max(film_timesteps) >= film_steps:
                raise ValueError("film_timesteps needs film_steps = T and timesteps in [0, T)")
            key += (("tau", film_timesteps),)
        P = self._cached_plan(self._plans, key, room=max(1, PLAN_CACHE_SIZE))
        if P is not None:
            return P
        if ctx_len + phosc_len == 0:
            raise NotImplementedError("context=None: every reference script conditions on the word (unet.py:1605)")
        if mix and self.model.num_classes is None:
            raise ValueError("writer-style interpolation needs a class-conditional model (num_classes)")
        if mix not in (0, 1, 2) or (mix == 2 and not film_steps):
            raise ValueError(f"mix = {mix}: 1 or 2 forwards per step with the table, 1 without")
        if (guide or writer_keep) and mix:
            raise NotImplementedError("writer-free guidance on top of writer-style interpolation (guide / writer_keep with mix)")
        if (guide or writer_keep) and self.model.num_classes is None:
            raise ValueError("writer-free guidance needs a class-conditional model (num_classes)")
        if guide not in (0, 2) or (guide and not film_steps) or (writer_keep and (film_steps or guide)):
            raise ValueError(f"guide = {guide}: two forwards per step with the table; writer_keep: the plan without the table")
        taps = self._map_taps(ctx_len + phosc_len) if attn_maps else ()  # (raises before anything is built or launched)
        P = self._begin_plan(Plan(), B)
        dev = self.device
        self._inputs(P, H, W, ctx_len, phosc_len)
        P.map_taps = taps
        self._conditioning(P, P.cond, ctx_len, phosc_len)  # step-invariant: run once per call (P.cond)
        P.mix, P.guide = mix, guide
        if mix:
            P.mix_m = torch.zeros((B,), dtype=torch.float32, device=dev)
        P.keep_in = torch.ones((B,), dtype=torch.uint8, device=dev) if writer_keep else None
        self._film = self._f32(P, B, self.film_total)
        P.t_dev = torch.zeros((1,), dtype=torch.int32, device=dev)
        P.k_dev = torch.zeros((1,), dtype=torch.int32, device=dev)  # index into film_timesteps (the table-driven loop)
        if attn_maps and attn_rows:
            P.map_w = torch.zeros((int(attn_rows),), dtype=torch.float32, device=dev)
            P.map_k = P.k_dev if attn_by_step else P.t_dev
        P.film = []
        # per step: time / label embedding (unet.py:1550-1581) + all emb_layers at once (unet.py:609-615,660) into self._film, ...
        select1 = self._film_table(P, film_steps, film_timesteps) if film_steps else self._film_per_step(P)
        # ... the first convolution, the blocks, the output convolution into P.out
        cur = self._head(P, H, W)
        cur = self._trunk(P, cur)
        self._tail(P, cur)
        if mix == 2 or guide == 2:
            self._second_forward(P, select1)
        self._plans[key] = P
        return P

    def _film_table(self, P: Plan, film_steps: int, film_timesteps: Optional[tuple]):
        """The tabulated FiLM path (``plan`` film_steps / film_timesteps): ``P.film`` evaluates the time MLP of every table row once
        per call, ``P.film_prepare`` makes the chunk of rows a step reads resident, and the step begins by selecting its rows.
        Returns the select op a second forward begins with (mix = 2 or guide = 2), else None."""
        lib, dev, B, mix, film = self.lib, self.device, self._B, P.mix, P.film
        mc = self.model.model_channels
        ted = 4 * mc
        # the table holds ``chunk`` consecutive timesteps (rows (t % chunk) * B + b), not all T: T*B*film_total fp32 was
        # 655 MB + 328 MB of operand planes at B = 64 and grew with B and T; a chunk of ~8192 rows is 84 + 42 MB at any
        # B.  The time MLP (T rows, cheap) is still evaluated for every t once per call (P.film); the SiLU(time + label)
        # planes and the emb_layers GEMM of a chunk run when the loop enters it (P.film_prepare, same stream, a fraction
        # of one step each).
        T = film_steps if film_timesteps is None else len(film_timesteps)  # rows of the table: all t, or the visited ones
        nf = max(1, mix, P.guide)  # tables (forwards per step with FiLM rows of their own); the resident rows are shared between them
        # (a table over all t keeps at least 8 timesteps resident; one over the visited steps is cut by rows alone)
        chunk = min(T, max(8 if film_timesteps is None else 1, FILM_CHUNK_ROWS // (B * nf)))
        nchunks = (T + chunk - 1) // chunk
        Tp = nchunks * chunk
        if film_timesteps is None:
            tt = torch.arange(Tp, dtype=torch.int64, device=dev)
        else:  # row k holds timestep tau[k]; the padding rows repeat the last one and are never selected
            tt = torch.tensor(film_timesteps + (film_timesteps[-1],) * (Tp - T), dtype=torch.int64, device=dev)
        P.keep.append(tt)
        te = self._planes(P, Tp, mc)
        film.append((lib.wd_timestep_embedding, (tt.data_ptr(), Tp, self._w["freqs"].data_ptr(), mc // 2, *self._hilo(te), mc),
                     "timestep_embedding[all t]"))
        e1 = self._planes(P, Tp, ted)
        self._gemm(film, "time_embed.0[all t]", [self._src(te, mc)], "te0.w", Tp, 1, bias=self._w["te0.b"], act=N.ACT_SILU,
                   out_pl=e1)
        tm = self._f32(P, Tp, ted)
        self._gemm(film, "time_embed.2[all t]", [self._src(e1, ted)], "te2.w", Tp, 1, bias=self._w["te2.b"], out_f32=tm,
                   out_ld=ted)
        e2 = self._planes(P, nf * chunk * B, ted)
        P.film_table = self._f32(P, nf * chunk * B, self.film_total)
        P.film_chunk, P.film_nchunks, P.film_loaded = chunk, nchunks, -1
        if mix:
            P.pairs = torch.zeros((nf, Tp, B, 2), dtype=torch.int32, device=dev)
        chunk_gemm = []
        self._gemm(chunk_gemm, "emb_layers(all)[chunk of t]", [self._src(e2, ted)], "film.w", nf * chunk * B, 1,
                   bias=self._w["film.b"], out_f32=P.film_table, out_ld=self.film_total)
        P.film_prepare = self._film_prepare(P, tm, e2, chunk, nf, chunk_gemm)
        row_dev = P.t_dev if film_timesteps is None else P.k_dev
        P.step.append((lib.wd_select_rows, (P.film_table.data_ptr(), row_dev.data_ptr(), B, self.film_total, chunk,
                                            self._film.data_ptr()), "film rows of step t"))
        if nf != 2:
            return None
        return (lib.wd_select_rows, (P.film_table[chunk * B].data_ptr(), row_dev.data_ptr(), B, self.film_total, chunk,
                                     self._film.data_ptr()), "film rows of step t, second forward")

    def _film_prepare(self, P: Plan, tm, e2, chunk, nf, chunk_gemm):
        """``P.film_prepare`` of a tabulated plan, a closure over it: tm fp32 [rows, ted] the time MLP's output, e2 the planes that
        take SiLU(time + label) of the resident chunk, chunk_gemm the emb_layers GEMM over them."""
        lib, B, mix, ted = self.lib, self._B, P.mix, tm.shape[1]
        has_lab = self.model.num_classes is not None
        lab = self._w["label"].data_ptr() if has_lab else None
        yin = P.y_in.data_ptr() if has_lab else None
        ncls = self.model.num_classes if has_lab else 0

        def film_prepare(t, stream):
            """Makes the FiLM rows of timestep ``t`` resident: (re)computes the chunk ``t // chunk`` unless it is loaded."""
            c = int(t) // chunk
            if c == P.film_loaded:
                return False
            if mix:
                for f in range(nf):  # table f: rows f*chunk*B.. of the planes, pairs[f][c*chunk..]
                    N.check(lib.wd_emb_combine_mix(tm.data_ptr() + 4 * c * chunk * ted, lab, P.pairs[f, c * chunk].data_ptr(),
                                                   P.mix_m.data_ptr(), ncls, chunk, B, ted,
                                                   *self._hilo(e2, 2 * f * chunk * B * ted), ted, stream),
                            "SiLU(time + blended label)[chunk of t]")
            else:
                N.check(lib.wd_emb_combine(tm.data_ptr() + 4 * c * chunk * ted, lab, yin, ncls, chunk, B, ted, *self._hilo(e2), ted,
                                           stream), "SiLU(time + label)[chunk of t]")
                if P.guide:  # table 1: the writer-free rows, SiLU(time) (no keep mask: no sample keeps its writer)
                    N.check(lib.wd_emb_combine_keep(tm.data_ptr() + 4 * c * chunk * ted, None, None, None, 0, chunk, B, ted,
                                                    *self._hilo(e2, 2 * chunk * B * ted), ted, stream),
                            "SiLU(time)[chunk of t]")
            Plan._run(chunk_gemm, stream)
            P.film_loaded = c
            return True

        return film_prepare

    def _film_per_step(self, P: Plan):
        """The embedding path evaluated in every step (no table): three B-row GEMMs into ``self._film``.  mix: the label term is
        the blend of each sample's pair of writers.  ``P.keep_in``: it is label[y_b] or zeros, per sample."""
        m, lib, dev, B, mix, step = self.model, self.lib, self.device, self._B, P.mix, P.step
        mc = m.model_channels
        ted = 4 * mc
        has_lab = m.num_classes is not None
        own_rows = bool(mix) or P.keep_in is not None  # the writer rows of this batch are computed, not gathered from the table by y
        if mix:
            # the blended rows [B, ted] (wd_label_mix) are the residual of the time_embed.2 GEMM, row b for sample b
            P.pairs = torch.zeros((B, 2), dtype=torch.int32, device=dev)
            lab_rows = self._f32(P, B, ted)
            id_rows = torch.arange(B, dtype=torch.int64, device=dev)
            P.keep.append(id_rows)
            step.append((lib.wd_label_mix, (self._w["label"].data_ptr(), P.pairs.data_ptr(), P.mix_m.data_ptr(), m.num_classes,
                                            B, ted, lab_rows.data_ptr()), "blended label rows"))
        if P.keep_in is not None:  # the same residual form: rows [B, ted] read with identity row ids
            lab_rows = self._f32(P, B, ted)
            id_rows = torch.arange(B, dtype=torch.int64, device=dev)
            P.keep.append(id_rows)
            step.append((lib.wd_label_rows_keep, (self._w["label"].data_ptr(), P.y_in.data_ptr(), m.num_classes, B, ted, None,
                                                  P.keep_in.data_ptr(), lab_rows.data_ptr(), None, None),
                         "kept label rows"))
        te = self._planes(P, B, mc)
        step.append((lib.wd_timestep_embedding, (P.t_in.data_ptr(), B, self._w["freqs"].data_ptr(), mc // 2, *self._hilo(te), mc),
                     "timestep_embedding"))
        e1 = self._planes(P, B, ted)
        self._gemm(step, "time_embed.0", [self._src(te, mc)], "te0.w", B, 1, bias=self._w["te0.b"], act=N.ACT_SILU,
                   out_pl=e1)
        e2 = self._planes(P, B, ted)  # SiLU(emb): the only form any consumer reads (emb_layers start with SiLU)
        self._gemm(step, "time_embed.2+label", [self._src(e1, ted)], "te2.w", B, 1, bias=self._w["te2.b"],
                   resid=(lab_rows if own_rows else self._w["label"]).data_ptr() if has_lab else None, resid_ld=ted if has_lab else 0,
                   resid_rows=(id_rows if own_rows else P.y_in).data_ptr() if has_lab else None, act=N.ACT_SILU, out_pl=e2)
        self._gemm(step, "emb_layers(all)", [self._src(e2, ted)], "film.w", B, 1, bias=self._w["film.b"],
                   out_f32=self._film, out_ld=self.film_total)

    def _head(self, P: Plan, H, W) -> Act:
        """The first convolution of the step, from ``P.x_in``."""
        m, lib, B = self.model, self.lib, self._B
        mc = m.model_channels
        if not (self.fuse_in and self.variant != "phosc" and lib.wd_conv3x3_in_supported(m.in_channels, H, W, mc) and mc % 32 == 0):
            return self._head_gemm(P, P.step, "input_blocks.0", P.x_in, "in")[0]
        # the 4-channel 3x3 as a direct fp32 convolution: no im2col planes, and the statistics partials of the consumer's
        # GroupNorm (32 groups) in the layout the GEMM's epilogue gives them
        h0 = self._f32(P, B * H * W, mc)
        stats = None
        if self.fuse_stats:
            nchunk = lib.wd_conv3x3_in_nchunk(H * W)
            part = torch.zeros((B, nchunk, 32, 2), dtype=torch.float64, device=self.device)
            P.keep.append(part)
            stats = (part, nchunk, mc // 32)
        P.step.append((lib.wd_conv3x3_in, (P.x_in.data_ptr(), B, m.in_channels, H, W, self._w["in.w.f32"].data_ptr(),
                                           self._w["in.b"].data_ptr(), mc, h0.data_ptr(), mc,
                                           stats[0].data_ptr() if stats else None, mc // 32), "input_blocks.0: conv3x3 from NCHW"))
        return Act(h0, mc, H, W, stats)

    def _tail(self, P: Plan, cur: Act):
        """GroupNorm + SiLU + the output convolution of the step, into ``P.out`` (NCHW)."""
        lib, B, oc = self.lib, self._B, self.model.out_channels
        P.out = torch.empty((B, oc, cur.h, cur.w), dtype=torch.float32, device=self.device)
        if not (self.fuse_out and lib.wd_gn_conv3x3_few_supported(cur.c, cur.w, oc) and cur.c % 32 == 0):
            self._tail_gemm(P, P.step, "out.conv", cur, 1e-5, nchw=P.out)
            return
        # GroupNorm + SiLU + the 320 -> 4 convolution + NCHW in one fp32 launch (as a GEMM it fills 4 of 64 tile columns)
        part, nchunk, pc = self._gn_stats(P, P.step, "out.gn", cur)
        P.step.append((lib.wd_gn_conv3x3_few,
                       (cur.t.data_ptr(), cur.c, B, cur.h, cur.w, cur.c, cur.c // 32, part.data_ptr(), nchunk, pc,
                        self._w["out.gn.g"].data_ptr(), self._w["out.gn.b"].data_ptr(), 1e-5, 1,
                        self._w["out.w.f32"].data_ptr(), self._w["out.b"].data_ptr(), oc, P.out.data_ptr()),
                       "out: GroupNorm + SiLU + conv3x3 -> NCHW"))

    def _second_forward(self, P: Plan, select1):
        """``P.step1`` (mix = 2 or guide = 2), the second forward of a step: its own FiLM rows, the same launches, the prediction kept
        beside the first one in ``P.out1``.  The attention maps accumulate over the first forward alone."""
        fn, args, what = P.step[-1]
        assert args[-1] == P.out.data_ptr(), what
        P.out1 = torch.empty_like(P.out)
        P.step1 = [select1] + [op for op in P.step[1:-1] if op[0] is not self.lib.wd_xattn_maps] + \
            [(fn, args[:-1] + (P.out1.data_ptr(),), what)]

    # ------------------------------------------------------------------------------------------ run
    def check_ids(self, context=None, y=None, phosc=None, need_y=True):
        """Host-side range check of every integer the kernels use as a table row: writer ids against ``num_classes``
        (``label_emb``, unet.py:1581), word / PHOSC ids against the rows of the character table (unet.py:860).  The
        reference raises an index error for such an id; a raw device read past the table could fault the GPU instead."""
        m = self.model
        vocab = int(m.word_emb.embedding.weight.shape[0]) if hasattr(m, "word_emb") else None
        checks = []
        if getattr(m, "num_classes", None) is not None:
            if y is None:
                if need_y:
                    raise ValueError("y (writer ids) is required: the model is class-conditional (unet.py:1555)")
            else:
                checks.append(("writer id (y)", y, m.num_classes))
        for what, ids in (("word id (context)", context), ("PHOSC id (phoscLabels)", phosc)):
            if ids is not None and vocab is not None and ids.numel():
                checks.append((what, ids, vocab))
        if not checks:
            return
        vals = [v for _, ids, _ in checks for v in (ids.min().long(), ids.max().long())]
        ext = torch.stack(vals).tolist() if len({v.device for v in vals}) == 1 else [int(v) for v in vals]  # one sync
        for i, (what, _, bound) in enumerate(checks):
            lo, hi = int(ext[2 * i]), int(ext[2 * i + 1])
            if lo < 0 or hi >= bound:
                raise IndexError(f"{what} out of range: [{lo}, {hi}] does not fit a table of {bound} rows")

    def check_pairs(self, pairs):
        """Host-side range check of the writer pairs of the interpolation path (any integer tensor [..., 2]); the reference's
        ``label_emb`` lookup raises an index error for such an id (unet.py:1567)."""
        nc = self.model.num_classes
        if nc is None:
            raise ValueError("writer-style interpolation needs a class-conditional model (num_classes)")
        lo, hi = int(pairs.min()), int(pairs.max())
        if lo < 0 or hi >= nc:
            raise IndexError(f"writer id (style pair) out of range: [{lo}, {hi}] does not fit a table of {nc} rows")

    def load_mix(self, P: Plan, pairs, mix_rate, check=True):
        """pairs: int tensor shaped like ``P.pairs`` up to its leading timestep padding ([mix, T, B, 2] with the table, [B, 2]
        without); mix_rate: fp32 [B]."""
        if check:
            self.check_pairs(pairs)
        if P.pairs.dim() == 4:
            P.pairs[:, :pairs.shape[1]].copy_(pairs, non_blocking=True)
        else:
            P.pairs.copy_(pairs, non_blocking=True)
        P.mix_m.copy_(mix_rate, non_blocking=True)

    def load_keep(self, P: Plan, writer_keep):
        """writer_keep: bool / uint8 [B] (nonzero: the sample keeps its writer term), or False: no sample does."""
        if writer_keep is False:
            P.keep_in.zero_()
        else:
            P.keep_in.copy_(check_writer_keep(writer_keep, P.keep_in.shape[0]), non_blocking=True)

    def load_inputs(self, P: Plan, x=None, t=None, context=None, y=None, phosc=None, check=True):
        if check:
            self.check_ids(context, y, phosc, need_y=False)
        if x is not None:
            P.x_in.copy_(x, non_blocking=True)
        if t is not None:
            P.t_in.copy_(t, non_blocking=True)
        if y is not None:
            P.y_in.copy_(y, non_blocking=True)
        if context is not None:
            P.ctx_in.copy_(context, non_blocking=True)
        if phosc is not None:
            P.phosc_in.copy_(phosc.to(torch.int32) if phosc.dtype != torch.int32 else phosc, non_blocking=True)

    def forward(self, x, t, context, y, phosc=None, mix=None, attn_maps=False, writer_keep=None):
        """writer_keep (``load_keep``): the writer term per sample; None: every sample keeps it, the plan without the argument.
        mix = (int pairs [B, 2], fp32 mix rates [B]): the writer term is the blend of each sample's pair and ``y`` is unused
        (unet.py:1558-1573).  attn_maps: returns (eps, [m_in, m_mid, m_out]), m_i fp32 [B, h_i, w_i, L]: the per-character
        attention maps of the three tapped SpatialTransformers (``plan``)."""
        self.refresh_weights()
        B, _, H, W = x.shape
        ctx_len = 0 if context is None else context.shape[1]
        phosc_len = 0 if phosc is None else phosc.shape[1]
        if mix is not None:
            self.check_pairs(mix[0])
            y = None
        if writer_keep is not None:
            if mix is not None or attn_maps:
                raise ValueError("writer_keep cannot be combined with writer-style interpolation (mix_rate) or return_attention")
            if writer_keep is not False:
                writer_keep = check_writer_keep(writer_keep, B)
        P = self.plan(B, H, W, ctx_len, phosc_len, mix=1 if mix is not None else 0, attn_maps=bool(attn_maps),
                      **(dict(writer_keep=True) if writer_keep is not None else {}))
        self.check_ids(context, y, phosc, need_y=mix is None)
        self.load_inputs(P, x, t, context, y, phosc, check=False)
        if writer_keep is not None:
            self.load_keep(P, writer_keep)
        if mix is not None:
            self.load_mix(P, mix[0], mix[1], check=False)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        P.run_cond(stream)
        P.run_step(stream)
        if attn_maps:
            return P.out.clone(), [mp.clone().reshape(B, mh, mw, -1) for mp, (mh, mw) in zip(P.maps, P.map_hw)]
        return P.out.clone()
