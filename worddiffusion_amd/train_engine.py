"""Training-step engine: the forward of ``engine.py`` with every intermediate kept, plus a hand-scheduled backward.

The reference trains with autograd over ~150 ATen modules (``train.py:287-293``: ``model(...)`` -> ``MSELoss`` ->
``loss.backward()``).  Here the backward is a static launch list, built once per input shape next to the forward list:

  * d(input) of every convolution / linear is ``wd_gemm`` again - over the planes of d(output), with the inverse gather
    table (``backward.conv_bwd_table``) and the weights repacked [C_in][tap][C_out] ("B:" entries of the weight cache);
  * d(weight) is ``wd_gemm`` with the token dimension as the reduction: both operands are transposed into split-bf16
    planes by ``wd_transpose_planes`` (rows ordered (c_in, tap), so the GEMM output IS the OIHW gradient) and the kernel's
    split-K spreads the long reduction over the chip;
  * GroupNorm(+SiLU), LayerNorm, attention over the <=16 context tokens, GEGLU, SiLU, nearest-x2 and the embeddings
    have their own kernels in ``csrc/wd_bwd.hip``; bias / FiLM / norm-parameter gradients are deterministic two-stage
    column sums (no float atomics anywhere: a replayed step is bit-identical).

Gradients land in persistent buffers that become ``param.grad`` (reference layout), so ``torch.optim.AdamW``, gradient
clipping, DDP-style all-reduce (``dist.GradAllReducer``) and ``optim.FusedAdamW`` all see what autograd would have given
them.  Forward + backward replay as one hipGraph.  Scope: the base ``unet.UNetModel`` (what ``train.py:403`` builds).
"""
from __future__ import annotations

import ctypes as C
import os
from collections import namedtuple
from typing import Callable, Dict, List, Optional

import torch

from . import _native as N
from . import dropout as DO
from .backward import conv_bwd_table
from .engine import Act, GatherTable, Plan, UNetEngine, _ptr, check_writer_keep
from .layers import DownsampleParams, ResBlockParams, SpatialTransformerParams, UpsampleParams


class TAct(Act):
    """Feature map + its gradient buffer (``g``) and whether the backward list has written it yet (``gw``)."""
    __slots__ = ("g", "gw")

    def __init__(self, t, c, h, w, stats=None):
        super().__init__(t, c, h, w, stats)
        self.g, self.gw = None, False


class TrainPlan(Plan):
    def __init__(self):
        super().__init__()
        self.bwd: List[tuple] = []
        self.dout: Optional[torch.Tensor] = None
        self.row_grad: Optional[torch.Tensor] = None  # frozen-trunk plan (plan_train rows): the fitted rows' gradient, fp32 [R, ted]
        # training dropout: the wd_dropout of every ResBlock with p > 0 (read by the host at launch or capture) and the device
        # row base they all point to - uint64 [1] kept as int64 bits -, so a captured step draws new masks when replayed
        self.dropouts: List[DO.WdDropout] = []
        self.row_base: Optional[torch.Tensor] = None
        # writer dropout (plan_train label_drop): the decision of the last forward, uint8 [B], written by wd_label_rows_keep; a
        # drawn one is keyed by a wd_dropout of its own in ``dropouts`` (same seed, same row base, the tag of dropout.label_tag)
        self.writer_keep: Optional[torch.Tensor] = None
        # the engine's count of training forwards when this plan's intermediates were last written (TrainEngine.claim_forward):
        # with the plan object, the identity of a forward that ``TrainEngine.backward`` checks
        self.serial = 0

    def set_dropout_seed(self, seed: int):
        for d in self.dropouts:
            d.seed = int(seed) & 0xFFFFFFFFFFFFFFFF

    def set_row_base(self, row_base: int):
        """Queues the write of the global row of sample 0 on the current stream (a no-op for a plan without dropout)."""
        if self.dropouts:
            v = int(row_base) & 0xFFFFFFFFFFFFFFFF
            self.row_base.fill_(v - (1 << 64) if v >= (1 << 63) else v)

    def run_bwd(self, stream, begin: int = 0, end: Optional[int] = None):
        self._run(self.bwd[begin:end], stream)


def _rup(x: int, m: int) -> int:
    return (x + m - 1) // m * m


# One destination of a data-gradient GEMM: t [rows, ld] (+)= d(out) . W[w_row_off : w_row_off + nrows]
Dx = namedtuple("Dx", "t ld acc w_row_off nrows")
# How a segment's weight gradient runs (_dw_form): dw - wd_dw, else transposed planes + wd_gemm; defer - in the grouped launch of
# its shape (_flush_dw); hw_out / hw_src - the positions per sample wd_dw is given.  DwItem: one waiting for that launch.
DwForm = namedtuple("DwForm", "dw defer hw_out hw_src")
DwItem = namedtuple("DwItem", "what dpl d_ld planes wg out_ld ftab")
# What _transformer keeps for its backward.  An attention: x the residual stream it read, n the planes of LayerNorm ``ln``, q the
# query rows (q | k | v rows of the spatial self-attention), o the attention's output planes, ko the offset of its K | V columns.
# A block: its attentions, then the feed-forward's input stream x3, norm3 planes, GEGLU pre-activation u, hidden planes ffh (ffi
# wide) and output planes xpl.  The transformer: input x, output, GroupNorm planes gpl, M tokens (hw per sample), inner channels.
_AttnRec = namedtuple("_AttnRec", "tag at x n q o ko self_attn ln")
_BlockRec = namedtuple("_BlockRec", "tb p attns x3 n3 u ffh ffi xpl")
_STRec = namedtuple("_STRec", "name mod x out gpl M hw inner blocks")


class BwdSeg:
    """One operand of out = sum_seg gather(planes_seg) . W_seg^T as ``_bwd_linear`` differentiates it: planes [2, rows, ld] of ``c``
    channels read through ``ntaps`` taps of the forward table ``ftab`` (None: row for row) over ``hw_src`` source positions per
    sample; ``wgrad`` [n, c * ntaps] in OIHW order or None (``wgrad_packed`` = (packed [n, ld_k], OIHW destination, c_in) for the
    im2col input convolution); ``wb`` names the data-gradient weight of the ``dx`` destinations (Dx), whose rows are ``dx_rows``
    output positions (``dx_hw`` per sample) through the inverse table ``btab`` (a GatherTable; ``ftab`` is the device tensor wd_dw reads)."""
    __slots__ = ("planes", "c", "ntaps", "hw_src", "ftab", "btab", "wb", "wgrad", "wgrad_packed", "dx", "dx_rows", "dx_hw")

    def __init__(self, planes, c, ntaps, hw_src, ftab=None, btab=None, wb=None, wgrad=None, wgrad_packed=None, dx=(), dx_rows=0,
                 dx_hw=0):
        self.planes, self.c, self.ntaps, self.hw_src, self.ftab, self.btab = planes, c, ntaps, hw_src, ftab, btab
        self.wb, self.wgrad, self.wgrad_packed, self.dx, self.dx_rows, self.dx_hw = wb, wgrad, wgrad_packed, dx, dx_rows, dx_hw


def linear_seg(planes, k: int, hw: int, wb: str, wgrad, d, m: int) -> BwdSeg:
    """A linear layer (one tap) over ``m`` rows of ``k`` channels whose data gradient goes to ``d`` [m, k]."""
    return BwdSeg(planes, k, 1, hw, wb=wb, wgrad=wgrad, dx=[Dx(d, k, 0, 0, k)], dx_rows=m, dx_hw=hw)


def conv3_seg(planes, c: int, ftab, btab, hw_src: int, wb: str, wgrad, dx: Dx, dx_rows: int, dx_hw: int) -> BwdSeg:
    """A 3x3 convolution read through the gather table ``ftab``; ``dx`` is written through ``btab``."""
    return BwdSeg(planes, c, 9, hw_src, ftab=ftab, btab=btab, wb=wb, wgrad=wgrad, dx=[dx], dx_rows=dx_rows, dx_hw=dx_hw)


class _Build:
    """What one ``plan_train`` build collects on its way: made when the build starts, dropped when it ends or raises."""

    def __init__(self, rows=None):
        self.rows = rows                        # frozen-trunk plan: the label_emb rows being fitted (None: everything trains)
        self.tape: List[Callable] = []          # the backward of every block, in forward order
        self.pw = set()                         # parameter-gradient buffers the backward list has written (_pacc)
        self.deferred, self.deferred_outs = [], {}  # wd_colsum_finish_multi entries per round; rounds taken per buffer
        self.gn_names: Dict[int, str] = {}      # id(GroupNorm) -> name of its packed weights
        self.done_at: Dict[int, int] = {}       # gradient buffer data_ptr -> index of the last closure that writes it
        self.closure = 0
        self.dkv = self.dfilm = None            # d(K | V of every cross-attention), d(FiLM rows)
        self.dw_pending: Dict[tuple, List[DwItem]] = {}  # weight gradients waiting for their group, by shape


class TrainEngine(UNetEngine):
    def __init__(self, model, variant: str):
        super().__init__(model, variant)
        # the weights-to-registers GEMM is no faster on the training forward (11.03-11.14 ms per step without it, 11.18-11.25 with it at the
        # end of round 3 - its fragment-major weight images now come out of the repack launch itself, so that is the kernels alone).
        # The fused feed-forward does not keep the hidden activations the backward pass needs.
        self.use_wdirect = os.environ.get("WDIFF_TRAIN_WDIRECT", "0") != "0"
        self.use_smallmap = os.environ.get("WDIFF_TRAIN_SMALLMAP", "1") != "0"   # (forward only; -0.085 ms per step)
        self.fuse_ff = self.fuse_proj = False
        self.fold_proj = False       # (the backward pass differentiates ff.net[2] and proj_out as the two layers they are)
        self.use_up_phases = False   # (the backward pass differentiates the 3x3 form)
        self.fuse_gn_in = 0
        self.use_dw = os.environ.get("WDIFF_TRAIN_DW", "1") != "0"  # weight gradients through wd_dw (csrc/wd_dw.hip) where it applies
        self.fuse_geglu_bwd = os.environ.get("WDIFF_FUSE_GEGLU_BWD", "1") != "0"  # GEGLU backward inside the d(out) preparation of ff1
        self.fuse_gn_bwd = os.environ.get("WDIFF_FUSE_GN_BWD", "1") != "0"  # GroupNorm backward in one pass (wd_gn_bwd_fused)
        self.dw_group_max = int(os.environ.get("WDIFF_DW_GROUP", "8"))  # single-tap layers of one shape per grouped launch (1: off)
        self._bs: Optional[_Build] = None            # the plan build in progress
        self._tplans: Dict[tuple, TrainPlan] = {}
        self._live: Optional[TrainPlan] = None       # the plan of the latest training forward: what ``backward`` differentiates
        self._serial = 0                             # training forwards so far (TrainPlan.serial)
        self._grad: Dict[int, torch.Tensor] = {}     # id(param) -> gradient buffer (possibly a view into a group)
        self._params: Dict[int, torch.nn.Parameter] = {}
        self._btabs: Dict[tuple, GatherTable] = {}
        self._scr: Dict[str, torch.Tensor] = {}
        self._arena = None
        self._arena_used = 0
        self.defer_bias_sums = os.environ.get("WDIFF_DEFER_BIAS", "1") != "0"
        # data-parallel overlap: the backward list is cut into NBUCKETS segments such that after segment j a PREFIX of the
        # gradient arena is final (the arena is carved in the order the backward list first writes the gradients, so a prefix
        # = the layers nearest the output) - TrainStep all-reduces that prefix while the next segment runs
        self.nbuckets = int(os.environ.get("WDIFF_GRAD_BUCKETS", "3"))
        self._carve_order: List[tuple] = []          # (data_ptr, arena offset, rounded numel) in carve order
        self._cut_closures: Optional[List[int]] = None  # closures after which a bucket ends (fixed by the first plan)
        # training dropout through model(...) under autograd: the mask key, and the global row of the next forward's sample 0
        # (advanced by the batch after every training forward); TrainStep keys its own steps (training.py)
        self.dropout_seed = 0
        self.dropout_row_base = 0
        self._layer_of: Optional[Dict[int, int]] = None  # id(ResBlock) -> dropout layer (dropout.layer_ids)

    def set_precision(self, mode: str):
        old = self.npass
        super().set_precision(mode)
        if self.npass != old and self._tplans:
            self._tplans.clear()
            self._scr = {k: v for k, v in self._scr.items() if isinstance(k, tuple)}

    # ------------------------------------------------------------------------------------------ weights
    def _recipes(self):
        R = super()._recipes()
        m = self.model
        we = m.word_emb
        cd = we.embedding.weight.shape[1]
        R.matrix("B:we.qkv.w", cd, 3 * cd)
        for i, l in enumerate((we.attention.linear_query, we.attention.linear_key, we.attention.linear_value)):
            R["B:we.qkv.w"].bwd(l.weight, col_off=i * cd)
        for name, mod in self._walk():
            if isinstance(mod, ResBlockParams):
                R.matrix("B:" + name + ".c1.w", mod.cin, 9 * mod.cout).bwd(mod.in_layers[2].weight)
                R.matrix("B:" + name + ".c2.w", mod.cout, 9 * mod.cout).bwd(mod.out_layers[3].weight)
                if mod.cin != mod.cout:
                    R.matrix("B:" + name + ".skip.w", mod.cin, mod.cout).bwd(mod.skip_connection.weight)
            elif isinstance(mod, (DownsampleParams, UpsampleParams)):
                conv = mod.op if isinstance(mod, DownsampleParams) else mod.conv
                R.matrix("B:" + name + ".w", mod.cin, 9 * mod.cout).bwd(conv.weight)
            elif isinstance(mod, SpatialTransformerParams):
                inner = mod.heads * mod.d_head
                R.matrix("B:" + name + ".pi.w", mod.ch, inner).bwd(mod.proj_in.weight)
                R.matrix("B:" + name + ".po.w", inner, mod.ch).bwd(mod.proj_out.weight)
                for d, tb in enumerate(mod.transformer_blocks):
                    p = f"{name}.tb{d}"
                    for tag, at in (("a1", tb.attn1), ("a2", tb.attn2)):
                        if tag == "a1" and self.variant == "phosc":  # spatial self-attention: fused q|k|v projection
                            R.matrix(f"B:{p}.a1.qkv.w", inner, 3 * inner)
                            for i, l in enumerate((at.to_q, at.to_k, at.to_v)):
                                R[f"B:{p}.a1.qkv.w"].bwd(l.weight, col_off=i * inner)
                        else:
                            R.matrix(f"B:{p}.{tag}.q.w", inner, inner).bwd(at.to_q.weight)
                        R.matrix(f"B:{p}.{tag}.o.w", inner, inner).bwd(at.to_out[0].weight)
                    ffi = tb.ff.net[2].in_features
                    # the training forward keeps the GEGLU pre-activation: plain [x | gate] row order (unet.py:128)
                    R.linear(p + ".ff1u", tb.ff.net[0].proj)
                    R.matrix("B:" + p + ".ff1.w", inner, 2 * ffi).bwd(tb.ff.net[0].proj.weight)
                    R.matrix("B:" + p + ".ff2.w", ffi, inner).bwd(tb.ff.net[2].weight)
        ted = m.time_embed[2].out_features
        R.matrix("B:film.w", ted, self.film_total)
        c0 = 0
        for l in self._film_mods:
            R["B:film.w"].bwd(l.weight, col_off=c0)
            c0 += l.weight.shape[0]
        R.matrix("B:kv.w", cd, self.kv_total)
        c0 = 0
        for at in self._kv_mods:
            for l in (at.to_k, at.to_v):
                R["B:kv.w"].bwd(l.weight, col_off=c0)
                c0 += l.weight.shape[0]
        R.matrix("B:te2.w", ted, ted).bwd(m.time_embed[2].weight)
        # C_out padded to 32 columns per tap (the gradient planes of a 4-channel map are 32 wide)
        R.matrix("B:out.w", m.out[2].in_channels, 9 * 32).bwd(m.out[2].weight, npad=32)
        return R

    # ------------------------------------------------------------------------------------------ gradient buffers
    def _carve(self, shape) -> torch.Tensor:
        """A zeroed slice of the flat gradient arena (so that data-parallel training all-reduces ONE buffer)."""
        if self._arena is None:
            total = sum(_rup(p.numel(), 64) for p in self.model.parameters())
            self._arena = torch.zeros(total, dtype=torch.float32, device=self.device)
            self._arena_used = 0
        n = 1
        for d in shape:
            n *= int(d)
        out = self._arena[self._arena_used:self._arena_used + n].view(shape)
        self._carve_order.append((out.data_ptr(), self._arena_used, _rup(n, 64)))
        self._arena_used += _rup(n, 64)
        assert self._arena_used <= self._arena.numel()
        return out

    def _pgrad(self, p: torch.nn.Parameter, shape=None) -> Optional[torch.Tensor]:
        """The gradient buffer of ``p`` (viewed as ``shape``) - or None in a frozen-trunk build, where no parameter has one: every
        emitter then leaves out the launches whose only product it would be."""
        if self._bs.rows is not None:
            return None
        if id(p) not in self._grad:
            self._grad[id(p)] = self._carve(tuple(p.shape))
            self._params[id(p)] = p
        return self._grad[id(p)] if shape is None else self._grad[id(p)].view(shape)

    def _pgroup(self, params: List[torch.nn.Parameter]) -> torch.Tensor:
        """One buffer whose row blocks are the gradients of ``params`` (weights the forward concatenates: all FiLM
        projections, every cross-attention's K/V, the word encoder's q/k/v).  None in a frozen-trunk build (_pgrad)."""
        if self._bs.rows is not None:
            return None
        key = ("group",) + tuple(id(p) for p in params)
        if key not in self._scr:
            tail = tuple(params[0].shape[1:])
            rows = sum(p.shape[0] for p in params)
            buf = self._carve((rows,) + tail)
            r0 = 0
            for p in params:
                self._grad[id(p)] = buf[r0:r0 + p.shape[0]]
                self._params[id(p)] = p
                r0 += p.shape[0]
            self._scr[key] = buf
        return self._scr[key]

    def _ppair(self, p0: torch.nn.Parameter, p1: torch.nn.Parameter) -> torch.Tensor:
        """[2, c] buffer: row 0 is p0's gradient, row 1 p1's (norm scale / shift pairs come out of one column sum).  None in a
        frozen-trunk build (_pgrad)."""
        if self._bs.rows is not None:
            return None
        key = ("pair", id(p0), id(p1))
        if key not in self._scr:
            buf = self._carve((2,) + tuple(p0.shape))
            for i, p in enumerate((p0, p1)):
                self._grad[id(p)] = buf[i]
                self._params[id(p)] = p
            self._scr[key] = buf
        return self._scr[key]

    def grad_arena(self) -> torch.Tensor:
        """All parameter gradients as one flat fp32 tensor (views of it are the ``param.grad``s)."""
        return self._arena[: self._arena_used]

    def _param_colsum(self, ops, what, src_ptr, ld, rows, c, out_ptr, acc):
        """out[0..c) (+)= column sums of src[rows, c] (row pitch ld) where ``out`` is a PARAMETER gradient, so nothing in the
        backward list reads it: deferred to the batched launches at the end of the list (``wd_colsum_finish_multi``), one
        launch per round.  A gradient with several writers (a norm shared by two attentions, the word encoder's projections
        run once per token group in the PHOSC variant) gets one entry per writer, in successive rounds.  ``src`` must stay
        intact until the end of the list (a plan-owned buffer, not a shared scratch)."""
        rnd = self._bs.deferred_outs.get(out_ptr, 0)
        if not self.defer_bias_sums or rows > 1024 or (acc and rnd == 0):
            # (acc and rnd == 0: an earlier, non-deferred op of this list already wrote the row - keep program order)
            self._colsum(ops, what, src_ptr, ld, rows, c, rows, out_ptr, c, acc)
            return
        self._bs.deferred_outs[out_ptr] = rnd + 1
        while len(self._bs.deferred) <= rnd:
            self._bs.deferred.append([])
        self._bs.deferred[rnd].append((src_ptr, out_ptr, rows, c, ld, 1 if (rnd or acc) else 0, 1.0, 0))

    def _flush_deferred(self, P):
        for rnd, entries in enumerate(self._bs.deferred):
            if not entries:
                continue
            table = torch.frombuffer((N.WdColsumEntry * len(entries))(*entries), dtype=torch.uint8).to(self.device)
            P.keep.append(table)
            P.bwd.append((self.lib.wd_colsum_finish_multi, (table.data_ptr(), len(entries), max(e[3] for e in entries)),
                          f"parameter-gradient column sums: deferred finishes (round {rnd})"))
        self._bs.deferred, self._bs.deferred_outs = [], {}

    def _pacc(self, t: torch.Tensor) -> int:
        """1 if the backward list has already written this parameter-gradient buffer (shared norm2), else 0."""
        k = t.data_ptr()
        acc = k in self._bs.pw
        self._bs.pw.add(k)
        self._bs.done_at[k] = self._bs.closure  # (a buffer with several writers is final after the last one)
        return int(acc)

    def _gacc(self, P, act: TAct):
        if act.g is None:
            act.g = self._f32(P, *act.t.shape)
        acc = act.gw
        act.gw = True
        return act.g, int(acc)

    def _dresid(self, P, name, x: TAct, dO: torch.Tensor, M):
        """The identity branch of out = f(x) + x: d(out) added to x's gradient, or copied where it is the first to write it."""
        g, acc = self._gacc(P, x)
        if acc:
            P.bwd.append((self.lib.wd_add, (g.data_ptr(), dO.data_ptr(), g.numel()), name + ":dresid"))
        else:
            P.bwd.append((self.lib.wd_copy2d, (g.data_ptr(), 4 * x.c, dO.data_ptr(), 4 * x.c, 4 * x.c, M), name + ":dresid"))

    def _scratch(self, key: str, numel: int, dtype) -> torch.Tensor:
        cur = self._scr.get(key)
        if cur is None or cur.numel() < numel:
            if cur is not None and self._tplans:
                raise RuntimeError("scratch grew after a plan was built")  # sized by _size_scratch before any use
            self._scr[key] = torch.zeros(numel, dtype=dtype, device=self.device)
        return self._scr[key]

    def _btable(self, h, w, mode) -> GatherTable:
        key = (h, w, mode)
        if key not in self._btabs:
            tab, ho, wo = conv_bwd_table(h, w, mode)
            self._btabs[key] = GatherTable(torch.from_numpy(tab).to(self.device), ho, wo, tab)  # (an inverse table: no width hint)
        return self._btabs[key]

    # ------------------------------------------------------------------------------------------ backward emitters
    def _colsum(self, ops, what, x_ptr, ld, rows, c, seg, out_ptr, out_ld, acc, scale=1.0):
        scr = self._cs_scratch
        nseg, nblk = (rows + seg - 1) // seg, (seg + 63) // 64
        assert nseg * nblk * c <= scr.numel(), (what, nseg, nblk, c)
        ops.append((self.lib.wd_colsum, (x_ptr, ld, rows, c, seg, out_ptr, out_ld, int(acc), float(scale), scr.data_ptr(),
                                         scr.numel()), what))

    def _gemm_dw(self, ops, what, doutT, nrows, xT, ncols, mpad, out: torch.Tensor, out_ld, acc):
        a = N.WdGemmArgs()
        s = N.WdSrc()
        s.hi, s.lo = doutT[0].data_ptr(), doutT[1].data_ptr()
        s.ld, s.c, s.ntaps, s.hw_src = mpad, mpad, 1, 0
        a.src[0] = s
        a.nsrc, a.npass = 1, self.npass
        a.w_hi, a.w_lo = xT[0].data_ptr(), xT[1].data_ptr()
        a.m, a.n, a.ktot, a.hw_out = nrows, ncols, mpad, 1
        a.out_f32, a.out_ld = out.data_ptr(), out_ld
        if acc:
            a.resid, a.resid_ld = out.data_ptr(), out_ld
        a.ksplit, a.ws, a.ws_floats = 0, self._ws.data_ptr(), self._ws.numel()
        self._give_tickets(a, nrows, ncols)
        self._cur_plan.keep.append(a)
        ops.append((self.lib.wd_gemm, (C.byref(a),), what))

    def _dw(self, ops, what, dpl, d_ld, planes, col_off, c, ftab, ntaps, hw_out, hw_src, M, n, out: torch.Tensor, out_ld, acc):
        a = N.WdDwArgs()
        a.d_hi, a.d_lo = self._hilo(dpl)
        a.x_hi, a.x_lo = self._hilo(planes, 2 * col_off)
        a.gather = _ptr(ftab)
        a.grad, a.grad_ld, a.ws, a.ws_floats = out.data_ptr(), out_ld, self._ws.data_ptr(), self._ws.numel()
        a.d_ld, a.x_ld, a.ntaps, a.hw_out, a.hw_src = d_ld, planes.shape[2], ntaps, hw_out, hw_src
        a.m, a.n, a.c, a.npass, a.accumulate, a.nslice = M, n, c, self.npass, int(bool(acc)), 0
        self._cur_plan.keep.append(a)
        ops.append((self.lib.wd_dw, (C.byref(a),), what))

    def _flush_dw(self, P):
        """Emits the weight-gradient launches put off by _bwd_linear: layers of one shape as ONE grouped wd_dw_group launch."""
        pend, self._bs.dw_pending = self._bs.dw_pending, {}
        for (M, n, c, hw, ntaps, hw_src, _), items in pend.items():
            ftab = items[0].ftab
            for lo in range(0, len(items), self.dw_group_max):
                grp = items[lo:lo + self.dw_group_max]
                if len(grp) == 1:
                    it = grp[0]
                    self._dw(P.bwd, it.what, it.dpl, it.d_ld, it.planes, 0, c, ftab, ntaps, hw, hw_src, M, n, it.wg, it.out_ld,
                             self._pacc(it.wg))
                    continue
                arr = (N.WdDwItem * len(grp))()
                for i, it in enumerate(grp):
                    arr[i].d_hi, arr[i].d_lo = self._hilo(it.dpl)
                    arr[i].x_hi, arr[i].x_lo = self._hilo(it.planes)
                    arr[i].grad, arr[i].grad_ld = it.wg.data_ptr(), it.out_ld
                    arr[i].d_ld, arr[i].x_ld, arr[i].accumulate = it.d_ld, it.planes.shape[2], self._pacc(it.wg)
                dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.device)
                a = N.WdDwArgs()
                a.ws, a.ws_floats = self._ws.data_ptr(), self._ws.numel()
                a.gather = _ptr(ftab)
                a.ntaps, a.hw_out, a.hw_src, a.m, a.n, a.c, a.npass, a.nslice = ntaps, hw, hw_src, M, n, c, self.npass, 0
                P.keep += [arr, dev, a]
                P.bwd.append((self.lib.wd_dw_group, (C.byref(a), C.cast(arr, C.c_void_p), dev.data_ptr(), len(grp)),
                              "dW group: " + ", ".join(it.what for it in grp)))

    def _bwd_linear(self, P, what, dout: torch.Tensor, M, n, hw_out, segs: List[BwdSeg], bias=(), film_off=None, npad=None,
                    geglu=None):
        """Backward of out[M, n] = sum_seg gather(planes_seg) . W_seg^T + bias (+ FiLM row vector), appended to ``P.bwd``: the pass
        over d(out), then per segment its data-gradient GEMMs and its weight gradient, then the bias / FiLM sums.
        geglu = (u, dh, inner): d(output) is the GEGLU projection's and is NOT materialised - wd_dout_prep_geglu derives its planes
        and column sums from the saved pre-activation and the gradient of the activation's output (dout is None then)."""
        npad = n if npad is None else npad
        bias = [b for b in bias if b is not None]  # (a frozen-trunk build has no bias gradient: _pgrad)
        forms = [self._dw_form(s, M, n, npad, hw_out) for s in segs]
        dpl, doutT, colpart = self._stage_dout(P, what, dout, M, n, npad, hw_out, segs, forms, bias, film_off, geglu)
        for si, (s, form) in enumerate(zip(segs, forms)):
            self._emit_dx(P.bwd, f"{what}:dX{si}", s, dpl, npad, hw_out)
            if s.wgrad is not None or s.wgrad_packed is not None:
                self._emit_dw(P.bwd, what, si, s, form, dpl, doutT, M, n, npad)
        self._emit_sums(P.bwd, what, dout, M, n, hw_out, colpart, bias, film_off)

    def _dw_form(self, s: BwdSeg, M, n, npad, hw_out) -> DwForm:
        """Weight gradients straight from the row-major planes (wd_dw: transposed LDS reads) wherever the shape allows; the rest goes
        through transposed copies of both operands and wd_gemm.  Single-tap layers wait for the others of their shape (one grouped
        launch at the end of the block's backward, _flush_dw); 3x3 layers join a group only where a launch of their own would run
        short token slices - the 4 x 16 level: < 16 units of 64 tokens per slice -; the two convolutions of a ResBlock there share
        a launch."""
        lib, taps, ws = self.lib, s.ntaps, self._ws.numel()
        hw_dw = hw_out if (hw_out % 64 == 0 and M % hw_out == 0) else 64
        hw, hw_src = (hw_out, s.hw_src) if s.ftab is not None else (hw_dw, hw_dw)
        dw = bool(self.use_dw and s.wgrad is not None and npad % 8 == 0 and s.planes.shape[2] % 8 == 0 and
                  (s.ftab is not None or taps == 1) and lib.wd_dw_supported(M, n, s.c, taps, hw) and
                  lib.wd_dw_slices(M, n, s.c, taps) * n * s.c * taps <= ws)
        short = taps == 1 or (M // 64) // max(1, lib.wd_dw_slices(M, n, s.c, taps)) < 16
        defer = bool(dw and self.dw_group_max > 1 and short and (taps == 1) == (s.ftab is None) and
                     lib.wd_dw_group_slices(M, n, s.c, taps, 2) * 2 * n * s.c * taps <= ws)
        return DwForm(dw, defer, hw, hw_src)

    def _stage_dout(self, P, what, dout, M, n, npad, hw_out, segs, forms, bias, film_off, geglu):
        """One pass over d(output), appended to ``P.bwd``: row-major planes ``dpl`` (data gradient, wd_dw), transposed planes
        ``doutT`` (wd_gemm weight gradient), per-64-row column sums ``colpart`` (bias / FiLM gradients, whenever the segments line
        up).  Returns the three buffers, None for what no one reads."""
        lib, mpad = self.lib, _rup(M, 64)
        need_dw = any((s.wgrad is not None and not f.dw) or s.wgrad_packed is not None for s, f in zip(segs, forms))
        need_dpl = any(s.dx for s in segs) or any(f.dw for f in forms)
        dpl = doutT = colpart = None
        if need_dpl and any(f.defer for f in forms):
            # the planes of a deferred weight gradient are read at the end of the block's backward: a buffer of their own
            dpl = torch.empty(2, M, npad, dtype=torch.bfloat16, device=self.device)
            P.keep.append(dpl)
        elif need_dpl:
            dpl = self._scratch("dpl", 2 * self._max_dpl, torch.bfloat16)[: 2 * M * npad].view(2, M, npad)
        if need_dw:
            doutT = self._scratch("doutT", 2 * self._max_doutT, torch.bfloat16)[: 2 * n * mpad].view(2, n, mpad)
        if (bool(bias) or film_off is not None) and (film_off is None or hw_out % 64 == 0):
            if bias and self.defer_bias_sums:
                # the bias-gradient finish of this layer runs in the one batched launch at the end of the backward list, so
                # its partial sums need a buffer of their own
                colpart = torch.empty((mpad // 64) * n, dtype=torch.float32, device=self.device)
                P.keep.append(colpart)
            else:
                colpart = self._scratch("colpart", self._max_colpart, torch.float32)
            assert (mpad // 64) * n <= colpart.numel(), what
        outs = (*self._hilo(dpl), _ptr(doutT[0]) if need_dw else None, _ptr(doutT[1]) if need_dw else None, _ptr(colpart))
        if geglu is not None:
            u, dh, inner = geglu
            assert dout is None and n == 2 * inner and npad == n and (colpart is not None or not bias) and film_off is None, what
            P.bwd.append((lib.wd_dout_prep_geglu, (u.data_ptr(), u.shape[1], dh.data_ptr(), dh.shape[1], M, inner, mpad, *outs),
                          what + ":prep(geglu bwd)"))
        elif need_dpl or need_dw or colpart is not None:
            P.bwd.append((lib.wd_dout_prep, (dout.data_ptr(), dout.shape[1], M, n, npad, mpad, *outs), what + ":prep(dout)"))
        return dpl, doutT, colpart

    def _emit_dx(self, ops, what, s: BwdSeg, dpl, npad, hw_out):
        """The data-gradient GEMMs of one segment: d(out) planes through the inverse table times the repacked weight."""
        for dx in s.dx:
            src = self._src(dpl, npad, s.ntaps, s.btab, hw_out if s.btab is not None else 0)
            self._gemm(ops, what, [src], s.wb, s.dx_rows, s.dx_hw, resid=dx.t.data_ptr() if dx.acc else None,
                       resid_ld=dx.ld if dx.acc else 0, out_f32=dx.t, out_ld=dx.ld, n=dx.nrows, w_row_off=dx.w_row_off)

    def _emit_dw(self, ops, what, si, s: BwdSeg, form: DwForm, dpl, doutT, M, n, npad):
        """The weight gradient of one segment in the form ``_dw_form`` chose: queued for its group, wd_dw, or transposed planes +
        wd_gemm (+ the OIHW permutation of the im2col input convolution)."""
        c, ntaps, ftab, planes, wg = s.c, s.ntaps, s.ftab, s.planes, s.wgrad
        k, mpad = ntaps * c, _rup(M, 64)
        if form.defer:
            key = (M, n, c, form.hw_out, ntaps, form.hw_src, ftab.data_ptr() if ftab is not None else 0)
            self._bs.dw_pending.setdefault(key, []).append(DwItem(f"{what}:dW{si}", dpl, npad, planes, wg, k, ftab))
            return
        if form.dw:
            self._dw(ops, f"{what}:dW{si}", dpl, npad, planes, 0, c, ftab, ntaps, form.hw_out, form.hw_src, M, n, wg, k,
                     self._pacc(wg))
            return
        xT = self._scratch("xT", 2 * self._max_xT, torch.bfloat16)[: 2 * k * mpad].view(2, k, mpad)
        hw_out = form.hw_out if ftab is not None else 0
        ops.append((self.lib.wd_transpose_planes,
                    (planes[0].data_ptr(), planes[1].data_ptr(), 0, planes.shape[2], c, _ptr(ftab), ntaps, hw_out,
                     s.hw_src if ftab is not None else 0, M, mpad, 1 if s.wgrad_packed is None else 0, xT[0].data_ptr(),
                     xT[1].data_ptr()), f"{what}:T(x{si})"))
        if s.wgrad_packed is not None:
            packed, dst, cin = s.wgrad_packed
            self._gemm_dw(ops, f"{what}:dW{si}", doutT, n, xT, k, mpad, packed, k, 0)
            ops.append((self.lib.wd_permute_dw, (packed.data_ptr(), k, n, cin, 9, dst.data_ptr()), f"{what}:dW{si}:oihw"))
            self._pacc(dst)
        else:
            self._gemm_dw(ops, f"{what}:dW{si}", doutT, n, xT, k, mpad, wg, k, self._pacc(wg))

    def _emit_sums(self, ops, what, dout, M, n, hw_out, colpart, bias, film_off):
        """FiLM gradient (per-sample column sums of d(out), read by the embedding path's backward) and bias gradients (their sum
        over the batch): finishes of ``colpart`` where the pass over d(out) left it, column sums otherwise."""
        src, ld, rows = (dout.data_ptr(), dout.shape[1], M) if dout is not None else (None, n, M)
        if film_off is not None:
            B = M // hw_out
            dfilm = self._bs.dfilm.data_ptr() + 4 * film_off
            if colpart is not None:
                ops.append((self.lib.wd_colsum_finish, (colpart.data_ptr(), hw_out // 64, n, B, dfilm, self.film_total, 0, 1.0),
                            what + ":dfilm"))
            else:
                self._colsum(ops, what + ":dfilm", src, ld, M, n, hw_out, dfilm, self.film_total, 0)
            src, ld, rows = dfilm, self.film_total, B
        for b in bias:
            if colpart is not None:  # the sum over its 64-row blocks
                self._param_colsum(ops, what + ":dbias", colpart.data_ptr(), n, _rup(M, 64) // 64, n, b.data_ptr(), self._pacc(b))
            else:
                self._colsum(ops, what + ":dbias", src, ld, rows, n, rows, b.data_ptr(), n, self._pacc(b))

    def _dropout_args(self, P, mod: ResBlockParams, p: float) -> DO.WdDropout:
        """The wd_dropout of ResBlock ``mod``: layer tag, threshold and scale fixed here, the seed set before every launch or
        capture (TrainPlan.set_dropout_seed), the row read on the device from the plan's row base."""
        if self._layer_of is None:
            ids = DO.layer_ids(self.model)
            self._layer_of = {id(m_): ids[n_ + "."] for n_, m_ in self.model.named_modules() if isinstance(m_, ResBlockParams)}
        d = DO.WdDropout()
        d.seed, d.row_base, d.row_base_dev = 0, 0, P.row_base.data_ptr()
        d.tag, d.thr, d.scale = DO.tag(self._layer_of[id(mod)]), DO.threshold(p), float(DO.scale(p))
        P.dropouts.append(d)
        return d

    def _gn_bwd(self, P, what, srcs: List[TAct], gn: torch.nn.GroupNorm, eps, silu, dz: torch.Tensor, dropout=None):
        """dropout: the wd_dropout the forward masked this norm's output with (one source) - dz is masked on load."""
        ops = P.bwd
        lib = self.lib
        B = self._B
        hw = srcs[0].h * srcs[0].w
        ctot = sum(s.c for s in srcs)
        cpg = ctot // 32
        gam, bet = gn.weight, gn.bias
        gw, gb = self._w[self._bs.gn_names[id(gn)] + ".g"], self._w[self._bs.gn_names[id(gn)] + ".b"]
        pair = self._ppair(bet, gam)  # [d beta | d gamma], the order of the planar sums; None: frozen, the sums stay in scratch
        # one pass (the workgroup keeps its tile of dy / xhat in LDS) where the shape allows, else statistics pass + apply pass
        fused = self.fuse_gn_bwd and all(lib.wd_gn_bwd_fused_supported(hw, s.c, cpg) for s in srcs)
        nb = 1 if fused else lib.wd_gn_bwd_nchunk(hw)
        off = 0
        accp = self._pacc(pair) if pair is not None else 0
        for s in srcs:
            part, nchunk, pc = s.stats
            sums = self._f32(P, B, nb, 2, s.c)
            common = (s.t.data_ptr(), s.c, dz.data_ptr(), ctot, off, B, hw, s.c, cpg, part.data_ptr(), nchunk, pc,
                      gw.data_ptr(), gb.data_ptr(), off, eps, int(silu), sums.data_ptr())
            g, acc = self._gacc(P, s)
            if dropout is not None:
                assert len(srcs) == 1, what
                dr = (C.byref(dropout),)
                if fused:
                    ops.append((lib.wd_gn_bwd_fused_dropout, common + (g.data_ptr(), s.c, acc) + dr, what + ":bwd+dropout"))
                else:
                    ops.append((lib.wd_gn_bwd_stats_dropout, common + dr, what + ":stats+dropout"))
                    ops.append((lib.wd_gn_bwd_apply_dropout, common + (g.data_ptr(), s.c, acc) + dr, what + ":apply+dropout"))
            elif fused:
                ops.append((lib.wd_gn_bwd_fused, common + (g.data_ptr(), s.c, acc), what + ":bwd"))
            else:
                ops.append((lib.wd_gn_bwd_stats, common, what + ":stats"))
                ops.append((lib.wd_gn_bwd_apply, common + (g.data_ptr(), s.c, acc), what + ":apply"))
            if pair is None:
                pass  # (the by-product sums stay in ``sums``)
            elif len(srcs) == 1:
                self._param_colsum(ops, what + ":dbeta|dgamma", sums.data_ptr(), 2 * s.c, B * nb, 2 * s.c, pair.data_ptr(), accp)
            else:
                self._param_colsum(ops, what + ":dbeta", sums.data_ptr(), 2 * s.c, B * nb, s.c, pair[0].data_ptr() + 4 * off, accp)
                self._param_colsum(ops, what + ":dgamma", sums.data_ptr() + 4 * s.c, 2 * s.c, B * nb, s.c,
                                   pair[1].data_ptr() + 4 * off, accp)
            off += s.c

    def _ln_bwd(self, P, what, x: torch.Tensor, rows, c, ln: torch.nn.LayerNorm, name, dy: torch.Tensor, dx: torch.Tensor,
                acc: int):
        ops = P.bwd
        lib = self.lib
        nblk = lib.wd_layernorm_bwd_nblk(rows)
        colpart = self._f32(P, nblk, 2, c)
        ops.append((lib.wd_layernorm_bwd, (x.data_ptr(), c, dy.data_ptr(), c, rows, c, self._w[name + ".g"].data_ptr(), 1e-5,
                                           dx.data_ptr(), c, int(acc), colpart.data_ptr()), what))
        pair = self._ppair(ln.weight, ln.bias)  # [d gamma | d beta], the order of colpart
        if pair is not None:
            self._param_colsum(ops, what + ":dgamma|dbeta", colpart.data_ptr(), 2 * c, nblk, 2 * c, pair.data_ptr(), self._pacc(pair))

    def _attn_bwd(self, P, what, q_ptr, ldq, k_ptr, ldk, v_ptr, ldv, dO: torch.Tensor, heads, nq, nk, d, scale, dq_ptr, lddq,
                  dkv_ptr, dkv_pitch_floats, want_dkv=True):
        """dq -> dq_ptr; [dK | dV] rows (b, j) -> dkv_ptr with the given row pitch (2*inner floats wide).  want_dkv False: nothing
        reads them (the context of a frozen trunk), so the short-key form leaves its partial sums where they are."""
        ops = P.bwd
        lib = self.lib
        B = self._B
        inner = heads * d
        if nk > 16:
            # long key sets (spatial self-attention, PHOSC context): dK | dV land in the destination rows directly
            need = lib.wd_attention_bwd_scratch_floats(B, heads, nq, nk)
            scr = self._scratch("attn_bwd", max(need, self._max_attn_scr), torch.float32)
            ops.append((lib.wd_attention_bwd, (q_ptr, ldq, k_ptr, ldk, v_ptr, ldv, dO.data_ptr(), dO.shape[1], B, heads, nq, nk, d,
                                               float(scale), dq_ptr, lddq, dkv_ptr, dkv_pitch_floats, dkv_ptr + 4 * inner,
                                               dkv_pitch_floats, scr.data_ptr(), scr.numel()), what))
            return
        nwg = lib.wd_attention_bwd_small_nwg(heads, nq, nk, d)
        if nwg <= 0:
            raise NotImplementedError(f"attention backward shape heads={heads} nq={nq} nk={nk} d={d}")
        part = self._f32(P, B, nwg, nk, 2, inner)
        ops.append((lib.wd_attention_bwd_small, (q_ptr, ldq, k_ptr, ldk, v_ptr, ldv, dO.data_ptr(), dO.shape[1], B, heads, nq, nk,
                                                 d, float(scale), dq_ptr, lddq, part.data_ptr(), None), what))
        if not want_dkv:
            return
        row = nk * 2 * inner
        tmp = self._f32(P, B, row)
        self._colsum(ops, what + ":dkv", part.data_ptr(), row, B * nwg, row, nwg, tmp.data_ptr(), row, 0)
        ops.append((lib.wd_copy2d, (dkv_ptr, 4 * dkv_pitch_floats, tmp.data_ptr(), 8 * inner, 8 * inner, B * nk),
                    what + ":dkv->slice"))

    # ------------------------------------------------------------------------------------------ blocks (fwd + tape)
    def _resblock(self, P, name, mod: ResBlockParams, srcs: List[TAct]) -> TAct:
        ops = P.step
        B = self._B
        h, w = srcs[0].h, srcs[0].w
        hw, M = h * w, B * h * w
        cin, cout = mod.cin, mod.cout
        tab = self._table(h, w, "same")
        need_raw = cin != cout
        # nn.Dropout(p) of out_layers (unet.py:616-623): on the planes conv2 reads, recomputed by the backward of the second norm
        # (a frozen trunk is evaluated as model.eval() evaluates it: no dropout whatever p the module carries)
        p_drop = DO.check_p(mod.out_layers[2].p) if self._bs.rows is None else 0.0
        drop = self._dropout_args(P, mod, p_drop) if p_drop > 0 else None
        cpg = cin // 32
        parts = None
        if any(s.c % cpg for s in srcs):
            # GroupNorm groups straddle the skip concat (never at 320+320): materialise it (unet.py:1750) and hand its
            # gradient back to the two halves at the end of the block's backward
            parts = srcs
            catt = self._f32(P, M, cin)
            coff = 0
            for s in parts:
                ops.append((self.lib.wd_copy2d, (catt.data_ptr() + 4 * coff, 4 * cin, s.t.data_ptr(), 4 * s.c, 4 * s.c, M),
                            name + ":concat"))
                coff += s.c
            srcs = [TAct(catt, cin, h, w)]
        a1, raw = self._gn(P, ops, name + ".gn1", srcs, name + ".gn1", 1e-5, True, want_raw=need_raw)
        h1t = self._f32(P, M, cout)
        g1 = self._gemm(ops, name + ".conv1", [self._src(a1, cin, 9, tab, hw)], name + ".c1.w", M, hw,
                        bias=self._w[name + ".c1.b"], rowvec=self._film.data_ptr() + 4 * self.film_off[name],
                        rowvec_ld=self.film_total, out_f32=h1t, out_ld=cout, want_stats=True)
        h1 = TAct(h1t, cout, h, w, g1.stats)
        a2, _ = self._gn(P, ops, name + ".gn2", [h1], name + ".gn2", 1e-5, True, dropout=drop)
        outt = self._f32(P, M, cout)
        if need_raw:
            g2 = self._gemm(ops, name + ".conv2+skip", [self._src(a2, cout, 9, tab, hw), self._src(raw, cin)],
                            name + ".c2.w", M, hw, bias=self._w[name + ".c2.b"], out_f32=outt, out_ld=cout,
                            want_stats=True)
        else:
            g2 = self._gemm(ops, name + ".conv2", [self._src(a2, cout, 9, tab, hw)], name + ".c2.w", M, hw,
                            bias=self._w[name + ".c2.b"], resid=srcs[0].t.data_ptr(), resid_ld=cout, out_f32=outt,
                            out_ld=cout, want_stats=True)
        out = TAct(outt, cout, h, w, g2.stats)
        self._bs.gn_names[id(mod.in_layers[0])] = name + ".gn1"
        self._bs.gn_names[id(mod.out_layers[0])] = name + ".gn2"

        def bwd():
            bops = P.bwd
            assert out.gw, name
            dO = out.g
            btab = self._btable(h, w, "same")
            da2 = self._f32(P, M, cout)
            segs = [conv3_seg(a2, cout, tab.dev, btab, hw, "B:" + name + ".c2.w", self._pgrad(mod.out_layers[3].weight, (cout, -1)),
                              Dx(da2, cout, 0, 0, cout), M, hw)]
            biases = [self._pgrad(mod.out_layers[3].bias)]
            if need_raw:
                dxs, coff = [], 0
                for s in srcs:
                    g, acc = self._gacc(P, s)
                    dxs.append(Dx(g, s.c, acc, coff, s.c))
                    coff += s.c
                segs.append(BwdSeg(raw, cin, 1, hw, wb="B:" + name + ".skip.w",
                                   wgrad=self._pgrad(mod.skip_connection.weight, (cout, cin)), dx=dxs, dx_rows=M, dx_hw=hw))
                biases.append(self._pgrad(mod.skip_connection.bias))
            else:
                self._dresid(P, name, srcs[0], dO, M)
            self._bwd_linear(P, name + ".conv2", dO, M, cout, hw, segs, bias=biases)
            self._gn_bwd(P, name + ".gn2", [h1], mod.out_layers[0], 1e-5, True, da2, dropout=drop)
            da1 = self._f32(P, M, cin)
            self._bwd_linear(P, name + ".conv1", h1.g, M, cout, hw,
                             [conv3_seg(a1, cin, tab.dev, btab, hw, "B:" + name + ".c1.w",
                                        self._pgrad(mod.in_layers[2].weight, (cout, -1)), Dx(da1, cin, 0, 0, cin), M, hw)],
                             bias=[self._pgrad(mod.in_layers[2].bias)], film_off=self.film_off[name])
            self._gn_bwd(P, name + ".gn1", srcs, mod.in_layers[0], 1e-5, True, da1)
            if parts is not None:
                coff = 0
                for s in parts:
                    g, acc = self._gacc(P, s)
                    dst = self._f32(P, M, s.c) if acc else g
                    bops.append((self.lib.wd_copy2d, (dst.data_ptr(), 4 * s.c, srcs[0].g.data_ptr() + 4 * coff, 4 * cin, 4 * s.c,
                                                      M), name + ":d(concat)"))
                    if acc:
                        bops.append((self.lib.wd_add, (g.data_ptr(), dst.data_ptr(), g.numel()), name + ":d(concat)+"))
                    coff += s.c

        self._bs.tape.append(bwd)
        return out

    def _resample(self, P, name, mod, x: TAct, mode: str, cskip: Optional[int] = None) -> TAct:
        """(cskip: what ``_trunk`` tells the inference planner about the Upsample's consumer - the training forward always runs the
        9-tap form, whose output is in raster order.)"""
        ops = P.step
        B = self._B
        tab = self._table(x.h, x.w, mode)
        ho, wo = tab.ho, tab.wo
        hw_in, M_in = x.h * x.w, B * x.h * x.w
        pl = self._planes(P, M_in, x.c)
        ops.append((self.lib.wd_split, (x.t.data_ptr(), x.c, M_in, x.c, 0, *self._hilo(pl), x.c), name + ":split"))
        outt = self._f32(P, B * ho * wo, mod.cout)
        gg = self._gemm(ops, name + ".conv", [self._src(pl, x.c, 9, tab, hw_in)], name + ".w", B * ho * wo, ho * wo,
                        bias=self._w[name + ".b"], out_f32=outt, out_ld=mod.cout, want_stats=True)
        out = TAct(outt, mod.cout, ho, wo, gg.stats)
        conv = mod.op if mode == "down" else mod.conv

        def bwd():
            bops = P.bwd
            assert out.gw, name
            M_out, hw_out = B * ho * wo, ho * wo
            g, acc = self._gacc(P, x)
            if mode == "down":
                btab = self._btable(x.h, x.w, "down")
                dx, dx_rows, dx_hw = Dx(g, x.c, acc, 0, x.c), M_in, hw_in
            else:  # nearest x2: data gradient at the upsampled resolution, then 2x2 sums
                btab = self._btable(ho, wo, "same")
                du = self._f32(P, M_out, x.c)
                dx, dx_rows, dx_hw = Dx(du, x.c, 0, 0, x.c), M_out, hw_out
            self._bwd_linear(P, name + ".conv", out.g, M_out, mod.cout, hw_out,
                             [conv3_seg(pl, x.c, tab.dev, btab, hw_in, "B:" + name + ".w", self._pgrad(conv.weight, (mod.cout, -1)),
                                        dx, dx_rows, dx_hw)],
                             bias=[self._pgrad(conv.bias)])
            if mode == "up":
                if acc:
                    tmp = self._f32(P, M_in, x.c)
                    bops.append((self.lib.wd_pool2x2_sum, (du.data_ptr(), B, x.h, x.w, x.c, tmp.data_ptr()), name + ":pool"))
                    bops.append((self.lib.wd_add, (g.data_ptr(), tmp.data_ptr(), g.numel()), name + ":pool+"))
                else:
                    bops.append((self.lib.wd_pool2x2_sum, (du.data_ptr(), B, x.h, x.w, x.c, g.data_ptr()), name + ":pool"))

        self._bs.tape.append(bwd)
        return out

    def _transformer(self, P, name, mod: SpatialTransformerParams, x: TAct) -> TAct:
        ops = P.step
        lib = self.lib
        B = self._B
        h, w, c = x.h, x.w, x.c
        hw, M = h * w, B * h * w
        heads, d = mod.heads, mod.d_head
        inner = heads * d
        L = self._ctx_len
        scale = d ** -0.5
        gpl, _ = self._gn(P, ops, name + ".gn", [x], name + ".gn", 1e-6, False)
        self._bs.gn_names[id(mod.norm)] = name + ".gn"
        tok = self._f32(P, M, inner)
        self._gemm(ops, name + ".proj_in", [self._src(gpl, c)], name + ".pi.w", M, hw, bias=self._w[name + ".pi.b"],
                   out_f32=tok, out_ld=inner)
        blocks = []
        cur = tok
        for di, tb in enumerate(mod.transformer_blocks):
            p = f"{name}.tb{di}"
            attns = []
            # base model: both attentions are cross-attentions reading norm2 (unet.py:337-345); PHOSC model: attn1 is the
            # spatial self-attention behind norm1 (unetPhosc.py:241-246)
            for tag, at in (("a1", tb.attn1), ("a2", tb.attn2)):
                self_attn = tag == "a1" and self.variant == "phosc"
                ln = "norm1" if self_attn else "norm2"
                n_pl = self._ln(P, ops, f"{p}.{ln}({tag})", cur, M, inner, f"{p}.{ln}")
                o = self._planes(P, M, inner)
                if self_attn:
                    qkv = self._f32(P, M, 3 * inner)
                    self._gemm(ops, p + ".a1.qkv", [self._src(n_pl, inner)], p + ".a1.qkv.w", M, hw, out_f32=qkv,
                               out_ld=3 * inner)
                    self._attention(ops, p + ".a1", qkv.data_ptr(), 3 * inner, qkv.data_ptr() + 4 * inner, 3 * inner,
                                    qkv.data_ptr() + 8 * inner, 3 * inner, heads, hw, hw, d, scale, o)
                    attns.append(_AttnRec(tag, at, cur, n_pl, qkv, o, 0, True, ln))
                else:
                    q = self._f32(P, M, inner)
                    self._gemm(ops, f"{p}.{tag}.q", [self._src(n_pl, inner)], f"{p}.{tag}.q.w", M, hw, out_f32=q, out_ld=inner)
                    ko = self.kv_off[f"{p}.{tag}"]
                    self._attention(ops, f"{p}.{tag}", q.data_ptr(), inner, self._kv.data_ptr() + 4 * ko, self.kv_total,
                                    self._kv.data_ptr() + 4 * (ko + inner), self.kv_total, heads, hw, L, d, scale, o)
                    attns.append(_AttnRec(tag, at, cur, n_pl, q, o, ko, False, ln))
                nxt = self._f32(P, M, inner)
                self._gemm(ops, f"{p}.{tag}.out", [self._src(o, inner)], f"{p}.{tag}.o.w", M, hw,
                           bias=self._w[f"{p}.{tag}.o.b"], resid=cur.data_ptr(), resid_ld=inner, out_f32=nxt, out_ld=inner)
                cur = nxt
            ffi = tb.ff.net[2].in_features
            n3 = self._ln(P, ops, p + ".norm3", cur, M, inner, p + ".norm3")
            u = self._f32(P, M, 2 * ffi)
            self._gemm(ops, p + ".ff1", [self._src(n3, inner)], p + ".ff1u.w", M, hw, bias=self._w[p + ".ff1u.b"], out_f32=u,
                       out_ld=2 * ffi)
            ffh = self._planes(P, M, ffi)
            ops.append((lib.wd_geglu_fwd, (u.data_ptr(), 2 * ffi, M, ffi, *self._hilo(ffh), ffi), p + ".geglu"))
            nxt = self._f32(P, M, inner)
            xpl = self._planes(P, M, inner)
            self._gemm(ops, p + ".ff2", [self._src(ffh, ffi)], p + ".ff2.w", M, hw, bias=self._w[p + ".ff2.b"],
                       resid=cur.data_ptr(), resid_ld=inner, out_f32=nxt, out_ld=inner, out_pl=xpl)
            blocks.append(_BlockRec(tb, p, attns, cur, n3, u, ffh, ffi, xpl))
            cur = nxt
        outt = self._f32(P, M, c)
        gg = self._gemm(ops, name + ".proj_out", [self._src(blocks[-1].xpl, inner)], name + ".po.w", M, hw,
                        bias=self._w[name + ".po.b"], resid=x.t.data_ptr(), resid_ld=c, out_f32=outt, out_ld=c,
                        want_stats=True)
        out = TAct(outt, c, h, w, gg.stats)

        st = _STRec(name, mod, x, out, gpl, M, hw, inner, blocks)

        def bwd():
            dcur = self._st_out_bwd(P, st)
            for blk in reversed(blocks):
                self._ff_bwd(P, st, blk, dcur)
                for a in reversed(blk.attns):
                    self._attn_layer_bwd(P, st, blk, a, dcur)
            self._st_in_bwd(P, st, dcur)

        self._bs.tape.append(bwd)
        return out

    def _st_out_bwd(self, P, st: _STRec) -> torch.Tensor:
        """out = proj_out(tokens) + x: d(out) into x's gradient, and through proj_out into the gradient of the running token
        stream (the residual adds of the blocks share it), which it returns."""
        name, mod, c, M = st.name, st.mod, st.x.c, st.M
        assert st.out.gw, name
        dO = st.out.g
        self._dresid(P, name, st.x, dO, M)
        dcur = self._f32(P, M, st.inner)
        self._bwd_linear(P, name + ".proj_out", dO, M, c, st.hw,
                         [linear_seg(st.blocks[-1].xpl, st.inner, st.hw, "B:" + name + ".po.w",
                                     self._pgrad(mod.proj_out.weight, (c, st.inner)), dcur, M)],
                         bias=[self._pgrad(mod.proj_out.bias)])
        return dcur

    def _ff_bwd(self, P, st: _STRec, blk: _BlockRec, dcur):
        """out = ff2(geglu(ff1(LN3(x3)))) + x3: dcur is d(out) and gets LN3's data gradient added."""
        tb, p, ffi, M, hw, inner = blk.tb, blk.p, blk.ffi, st.M, st.hw, st.inner
        dffh = self._f32(P, M, ffi)
        self._bwd_linear(P, p + ".ff2", dcur, M, inner, hw,
                         [linear_seg(blk.ffh, ffi, hw, "B:" + p + ".ff2.w", self._pgrad(tb.ff.net[2].weight), dffh, M)],
                         bias=[self._pgrad(tb.ff.net[2].bias)])
        dn3 = self._f32(P, M, inner)
        ff1_seg = [linear_seg(blk.n3, inner, hw, "B:" + p + ".ff1.w", self._pgrad(tb.ff.net[0].proj.weight), dn3, M)]
        # fused: d(GEGLU pre-activation) goes straight to operand planes + bias column sums (never written as fp32)
        fused, du = self.fuse_geglu_bwd and ffi % 64 == 0, None
        if not fused:
            du = self._f32(P, M, 2 * ffi)
            P.bwd.append((self.lib.wd_geglu_bwd, (blk.u.data_ptr(), 2 * ffi, dffh.data_ptr(), ffi, M, ffi, du.data_ptr(), 2 * ffi),
                          p + ".geglu:bwd"))
        self._bwd_linear(P, p + ".ff1", du, M, 2 * ffi, hw, ff1_seg, bias=[self._pgrad(tb.ff.net[0].proj.bias)],
                         geglu=(blk.u, dffh, ffi) if fused else None)
        self._ln_bwd(P, p + ".norm3:bwd", blk.x3, M, inner, tb.norm3, p + ".norm3", dn3, dcur, 1)

    def _attn_layer_bwd(self, P, st: _STRec, blk: _BlockRec, a: _AttnRec, dcur):
        """out = to_out(attention(q(LN(x)), K, V)) + x, self or cross: dcur is d(out) and gets the LayerNorm's data gradient added;
        a cross-attention leaves d(K | V) in its columns of the build's ``dkv``."""
        p, tag, at, M, hw, inner = blk.p, a.tag, a.at, st.M, st.hw, st.inner
        heads, d = st.mod.heads, st.mod.d_head
        do = self._f32(P, M, inner)
        self._bwd_linear(P, f"{p}.{tag}.out", dcur, M, inner, hw,
                         [linear_seg(a.o, inner, hw, f"B:{p}.{tag}.o.w", self._pgrad(at.to_out[0].weight), do, M)],
                         bias=[self._pgrad(at.to_out[0].bias)])
        dn = self._f32(P, M, inner)
        if a.self_attn:  # q holds the q | k | v rows, dq their gradient
            proj, dq, q = "a1.qkv", self._f32(P, M, 3 * inner), a.q.data_ptr()
            self._attn_bwd(P, f"{p}.a1:bwd", q, 3 * inner, q + 4 * inner, 3 * inner, q + 8 * inner, 3 * inner, do, heads, hw, hw, d,
                           d ** -0.5, dq.data_ptr(), 3 * inner, dq.data_ptr() + 4 * inner, 3 * inner)
            wg = self._pgroup([at.to_q.weight, at.to_k.weight, at.to_v.weight])
        else:
            proj, dq = tag + ".q", self._f32(P, M, inner)
            kv, dkv = self._kv.data_ptr() + 4 * a.ko, self._bs.dkv.data_ptr() + 4 * a.ko
            self._attn_bwd(P, f"{p}.{tag}:bwd", a.q.data_ptr(), inner, kv, self.kv_total, kv + 4 * inner, self.kv_total, do, heads,
                           hw, self._ctx_len, d, d ** -0.5, dq.data_ptr(), inner, dkv, self.kv_total,
                           want_dkv=self._bs.rows is None)
            wg = self._pgrad(at.to_q.weight)
        self._bwd_linear(P, f"{p}.{proj}", dq, M, dq.shape[1], hw, [linear_seg(a.n, inner, hw, f"B:{p}.{proj}.w", wg, dn, M)])
        self._ln_bwd(P, f"{p}.{a.ln}({tag}):bwd", a.x, M, inner, getattr(blk.tb, a.ln), f"{p}.{a.ln}", dn, dcur, 1)

    def _st_in_bwd(self, P, st: _STRec, dcur):
        """tokens = proj_in(GroupNorm(x)): dcur through proj_in and the norm into x's gradient."""
        name, mod, c, M = st.name, st.mod, st.x.c, st.M
        dg = self._f32(P, M, c)
        self._bwd_linear(P, name + ".proj_in", dcur, M, st.inner, st.hw,
                         [linear_seg(st.gpl, c, st.hw, "B:" + name + ".pi.w", self._pgrad(mod.proj_in.weight, (st.inner, c)),
                                     dg, M)], bias=[self._pgrad(mod.proj_in.bias)])
        self._gn_bwd(P, name + ".gn", [st.x], mod.norm, 1e-6, False, dg)

    # ------------------------------------------------------------------------------------------ plan
    def _size_scratch(self, B, H, W, L, ctx_len=0, phosc_len=0):
        m = self.model
        mc = m.model_channels
        cmax = mc * max(m.channel_mult)
        M = max(B * H * W, B * L)
        mpad = _rup(M, 64)
        nmax = max(8 * cmax, self.film_total, self.kv_total, 4 * mc)        # widest d(output): GEGLU pre-activation
        kmax = max(9 * 2 * cmax, 4 * cmax, 4 * mc, self.kpad_in)           # longest (tap, channel) list: 3x3 over a concat
        self._max_dpl = M * nmax
        self._max_doutT = nmax * mpad
        self._max_xT = kmax * mpad
        heads_max = max([mod.heads for _, mod in self._walk() if isinstance(mod, SpatialTransformerParams)] or [1])
        scr = 0
        if self.variant == "phosc" and H * W > 16:
            scr = max(scr, 2 * B * heads_max * (H * W) ** 2)
        if L > 16:
            scr = max(scr, 2 * B * heads_max * H * W * L)
        for n_tok in (ctx_len, phosc_len):
            if n_tok > 16:
                scr = max(scr, 2 * B * n_tok * n_tok)
        self._max_attn_scr = scr
        if scr:
            self._scratch("attn_bwd", scr, torch.float32)
        self._max_colpart = (mpad // 64) * nmax
        self._scratch("colpart", self._max_colpart, torch.float32)
        self._scratch("dpl", 2 * self._max_dpl, torch.bfloat16)
        self._scratch("doutT", 2 * self._max_doutT, torch.bfloat16)
        self._scratch("xT", 2 * self._max_xT, torch.bfloat16)
        self._cs_scratch = self._scratch("colsum", max(1 << 22, (M // 64 + 1) * nmax), torch.float32)
        if self._ws is None or self._ws.numel() < 8 * 2 * cmax * 9 * cmax:
            self._ws = torch.empty(max(128 * 128 * 160 * 8, 8 * 2 * cmax * 9 * cmax), dtype=torch.float32, device=self.device)

    def plan_train(self, B: int, H: int, W: int, ctx_len: int, phosc_len: int = 0, label_drop=None, rows=None) -> TrainPlan:
        """rows: None - everything trains, the plan without the argument; a tuple of distinct writer ids - the frozen-trunk plan
        that fits those rows of ``label_emb`` (DESIGN.md "Fitting new writers").  Its forward is the training forward WITHOUT
        ResBlock dropout, whatever p the modules carry: a frozen trunk is evaluated as ``model.eval()`` evaluates it.  Its backward
        is the full list minus every launch whose only product is the gradient of a frozen parameter - the data-gradient chain
        down to the FiLM rows, emb_layers(all)'s dX and the embedding SiLU stay -, then ``wd_row_slots`` on the plan's ``y`` and
        ``wd_embedding_bwd`` into ``P.row_grad``, compact fp32 [len(rows), ted].  No buffer of the gradient arena is carved or
        written and there are no bucket cuts.
        label_drop: None - every sample keeps its writer term, the plan without the argument; "mask" - the term per sample from
        ``P.keep_in`` (uint8 [B], ``load_keep``); a float p in (0, 1) - dropped with probability p, drawn on the device per
        global sample row (``wd_label_rows_keep``).  Either way the rows the kernel writes are the residual of the time_embed.2
        GEMM and label_emb's backward reads the ids it writes (-1 for a dropped sample: no gradient row)."""
        key, label_drop, rows = self._train_key(B, H, W, ctx_len, phosc_len, label_drop, rows)
        P = self._cached_plan(self._tplans, key)
        if P is not None:
            return P
        if self._tplans:
            # scratch buffers and the gradient-accumulate flags are sized / decided per plan: one live shape at a time
            self._tplans.clear()
            self._scr = {k: v for k, v in self._scr.items() if isinstance(k, tuple)}
        m = self.model
        P = self._begin_plan(TrainPlan(), B)
        self._bs = _Build(rows)
        try:
            P.row_base = torch.zeros(1, dtype=torch.int64, device=self.device)
            L = ctx_len + phosc_len
            self._size_scratch(B, H, W, L, ctx_len, phosc_len)
            self._inputs(P, H, W, ctx_len, phosc_len)
            # the conditioning path is differentiated, so it is part of every step
            groups = self._conditioning(P, P.step, ctx_len, phosc_len)
            self._bs.dkv = self._f32(P, B * L, self.kv_total)
            emb = self._embed_fwd(P, label_drop)
            # head, trunk, tail: the GEMM forms, whose operand planes the backward list reads
            head, xin = self._head_gemm(P, P.step, "input_blocks.0", P.x_in, "in")
            first = TAct(head.t, m.model_channels, H, W, head.stats)
            last = self._trunk(P, first)
            self._bs.gn_names[id(m.out[0])] = "out.gn"
            P.out = torch.empty((B, m.out_channels, last.h, last.w), dtype=torch.float32, device=self.device)
            gpl, _ = self._tail_gemm(P, P.step, "out.conv", last, 1e-5, nchw=P.out)
            self._tail_bwd(P, last, gpl)
            self._replay_tape(P)
            self._embed_bwd(P, first, xin, emb)
            if rows is None:
                self._cond_bwd(P, groups, L)
            self._flush_dw(P)
            self._flush_deferred(P)
            P.bwd_segments = self._arena_segments(P) if rows is None else []
        finally:
            self._bs = None
        self._tplans[key] = P
        return P

    def _train_key(self, B, H, W, ctx_len, phosc_len, label_drop, rows=None):
        """Refuses what cannot train and returns (cache key, label_drop and rows as the plan takes them).  No device work and no
        change to the engine: a refused call leaves the cached plans as they were."""
        if rows is not None:  # the frozen-trunk plan: no dropout, so no p in its key
            if self.model.num_classes is None:
                raise ValueError("fitting writer rows needs a class-conditional model (num_classes)")
            if label_drop is not None:
                raise ValueError("a row being fitted must keep its writer term: rows together with label_drop")
            from .optim import check_rows
            rows = check_rows(rows, self.model.num_classes)
            key = (B, H, W, ctx_len, phosc_len, self.npass, ("rows", rows))
        else:
            # p outside [0, 1) cannot train (nn.Dropout itself accepts p = 1); a plan is built for its p's
            drops = tuple(DO.check_p(mod.out_layers[2].p) for _, mod in self._walk() if isinstance(mod, ResBlockParams))
            key = (B, H, W, ctx_len, phosc_len, self.npass) + ((drops,) if any(drops) else ())
        if label_drop is not None:
            if label_drop != "mask":
                label_drop = DO.check_p(label_drop)
                if label_drop == 0.0:
                    raise ValueError("label_drop = 0 is the plan without the argument: pass None")
            if self.model.num_classes is None:
                raise ValueError("writer dropout needs a class-conditional model (num_classes)")
            key += (("label_drop", label_drop),)
        if ctx_len == 0:
            raise NotImplementedError("context=None: every reference script conditions on the word (unet.py:1605)")
        if phosc_len and self.variant != "phosc":
            raise ValueError("phoscLabels are an input of UNetModelPhosc only")
        if self.model.out_channels > 32:
            raise NotImplementedError("out_channels > 32")  # (the gradient planes of the output convolution are 32 wide)
        return key, label_drop, rows

    def _embed_fwd(self, P, label_drop):
        """Appends the time / writer embedding and all FiLM projections (into ``self._film``) to ``P.step``, with the writer-dropout
        launch in front of time_embed.2 for a plan with ``label_drop``.  Returns what ``_embed_bwd`` reads: the planes and SiLU
        pre-activations (te, pre1, e1, pre2, e2) and the writer ids of label_emb's backward."""
        m, lib, B, dev, step = self.model, self.lib, self._B, self.device, P.step
        mc, ted = m.model_channels, 4 * m.model_channels
        te = self._planes(P, B, mc)
        step.append((lib.wd_timestep_embedding, (P.t_in.data_ptr(), B, self._w["freqs"].data_ptr(), mc // 2, *self._hilo(te), mc),
                     "timestep_embedding"))
        pre1 = self._f32(P, B, ted)
        self._gemm(step, "time_embed.0", [self._src(te, mc)], "te0.w", B, 1, bias=self._w["te0.b"], out_f32=pre1, out_ld=ted)
        e1 = self._planes(P, B, ted)
        step.append((lib.wd_split, (pre1.data_ptr(), ted, B, ted, 1, *self._hilo(e1), ted), "time_embed.1(SiLU)"))
        has_lab = m.num_classes is not None
        lab, lab_rows, y_bwd = (self._w["label"], P.y_in, P.y_in) if has_lab else (None, None, None)
        if label_drop is not None:
            # the writer rows of the batch, label[y_b] or zeros, read with identity row ids (the residual form of wd_label_mix)
            lab = self._f32(P, B, ted)
            lab_rows = torch.arange(B, dtype=torch.int64, device=dev)
            y_bwd = torch.zeros((B,), dtype=torch.int64, device=dev)
            P.writer_keep = torch.ones((B,), dtype=torch.uint8, device=dev)
            P.keep += [lab_rows, y_bwd]
            d = None
            if label_drop == "mask":
                P.keep_in = torch.ones((B,), dtype=torch.uint8, device=dev)
            else:
                d = DO.WdDropout()
                d.seed, d.row_base, d.row_base_dev = 0, 0, P.row_base.data_ptr()
                d.tag, d.thr, d.scale = DO.label_tag(), DO.threshold(label_drop), 1.0
                P.dropouts.append(d)
            step.append((lib.wd_label_rows_keep, (self._w["label"].data_ptr(), P.y_in.data_ptr(), m.num_classes, B, ted,
                                                  C.byref(d) if d is not None else None,
                                                  P.keep_in.data_ptr() if d is None else None, lab.data_ptr(), y_bwd.data_ptr(),
                                                  P.writer_keep.data_ptr()), "kept label rows"))
        pre2 = self._f32(P, B, ted)
        self._gemm(step, "time_embed.2+label", [self._src(e1, ted)], "te2.w", B, 1, bias=self._w["te2.b"],
                   resid=lab.data_ptr() if has_lab else None, resid_ld=ted if has_lab else 0,
                   resid_rows=lab_rows.data_ptr() if has_lab else None, out_f32=pre2, out_ld=ted)
        e2 = self._planes(P, B, ted)
        step.append((lib.wd_split, (pre2.data_ptr(), ted, B, ted, 1, *self._hilo(e2), ted), "emb_layers.0(SiLU)"))
        self._film = self._f32(P, B, self.film_total)
        self._bs.dfilm = self._f32(P, B, self.film_total)
        self._gemm(step, "emb_layers(all)", [self._src(e2, ted)], "film.w", B, 1, bias=self._w["film.b"], out_f32=self._film,
                   out_ld=self.film_total)
        return te, pre1, e1, pre2, e2, y_bwd

    def _tail_bwd(self, P, last: TAct, gpl):
        """Opens ``P.bwd``: d(out) (``P.dout``, NCHW) into token rows, the output convolution's backward, out.gn's backward."""
        m, B = self.model, self._B
        oc, Mo, hwo = m.out_channels, B * last.h * last.w, last.h * last.w
        tab = self._table(last.h, last.w, "same")
        P.dout = torch.zeros((B, oc, last.h, last.w), dtype=torch.float32, device=self.device)
        dtok = torch.zeros((Mo, 32), dtype=torch.float32, device=self.device)  # columns >= oc stay zero
        P.keep.append(dtok)
        P.bwd.append((self.lib.wd_nchw_to_tokens, (P.dout.data_ptr(), B, oc, hwo, dtok.data_ptr(), 32), "d(out):tokens"))
        dg = self._f32(P, Mo, last.c)
        self._bwd_linear(P, "out.conv", dtok, Mo, oc, hwo,
                         [conv3_seg(gpl, last.c, tab.dev, self._btable(last.h, last.w, "same"), hwo, "B:out.w",
                                    self._pgrad(m.out[2].weight, (oc, -1)), Dx(dg, last.c, 0, 0, last.c), Mo, hwo)],
                         bias=[self._pgrad(m.out[2].bias)], npad=32)
        self._gn_bwd(P, "out.gn", [last], m.out[0], 1e-5, True, dg)

    def _replay_tape(self, P):
        """Appends the backward of every block to ``P.bwd``, last block first, and sets ``P.bwd_cuts``.  Closures = units of the
        backward list (a layer each); bucket boundaries fall between closures, where the deferred column sums collected so far are
        finished, so that every gradient written up to there is final."""
        # (bytes the backward pass will write: the dead heads of the reference - res.*, wrd_proj, attnc, to_kv, norm1 of the base
        # model - never get a gradient; this only balances the buckets, correctness does not depend on it)
        def _live(name):
            return not (name.startswith("res.") or name.startswith("wrd_proj.") or ".attnc." in name or ".to_kv." in name or
                        (self.variant == "base" and ".norm1." in name))
        bs = self._bs
        if bs.rows is not None:  # no parameter gradient, so no arena prefix to finish: no cuts
            P.bwd_cuts = []
            for fn in reversed(bs.tape):
                fn()
            return
        total = sum(_rup(p.numel(), 64) for n_, p in self.model.named_parameters() if _live(n_))
        first_plan = self._cut_closures is None
        cuts_seen: List[int] = []
        P.bwd_cuts = []  # [(index into P.bwd where the segment ends, closure index)]
        bs.closure = 1
        for fn in reversed(bs.tape):
            fn()
            self._flush_dw(P)
            want = (first_plan and self.nbuckets > 1 and len(cuts_seen) < self.nbuckets - 1 and
                    self._arena_used >= (len(cuts_seen) + 1) * total // self.nbuckets) or \
                   (not first_plan and bs.closure in self._cut_closures)
            if want:
                self._flush_deferred(P)
                cuts_seen.append(bs.closure)
                P.bwd_cuts.append((len(P.bwd), bs.closure))
            bs.closure += 1
        if first_plan:
            self._cut_closures = cuts_seen

    def _embed_bwd(self, P, first: TAct, xin, emb):
        """Appends to ``P.bwd``: the input convolution's weight / bias gradient, then the FiLM projections, the time MLP and the
        writer embedding, from d(FiLM rows) back to the timestep embedding.  A frozen-trunk build keeps only the chain to the
        writer rows: emb_layers(all)'s data gradient, the embedding SiLU, then the row slots and the scatter into ``P.row_grad``."""
        m, lib, B, bops = self.model, self.lib, self._B, P.bwd
        te, pre1, e1, pre2, e2, y_bwd = emb
        mc, ted = m.model_channels, 4 * m.model_channels
        assert first.gw
        rows = self._bs.rows
        if rows is None:
            hw = first.h * first.w
            packed = self._f32(P, mc, self.kpad_in)
            self._bwd_linear(P, "input_blocks.0", first.g, B * hw, mc, hw,
                             [BwdSeg(xin, self.kpad_in, 1, hw,
                                     wgrad_packed=(packed, self._pgrad(m.input_blocks[0][0].weight), m.in_channels))],
                             bias=[self._pgrad(m.input_blocks[0][0].bias)])
        film_w = self._pgroup([l.weight for l in self._film_mods])
        film_b = self._pgroup([l.bias for l in self._film_mods])
        de2 = self._f32(P, B, ted)
        self._bwd_linear(P, "emb_layers(all)", self._bs.dfilm, B, self.film_total, 1,
                         [linear_seg(e2, ted, 1, "B:film.w", film_w, de2, B)], bias=[film_b])
        dpre2 = self._f32(P, B, ted)
        bops.append((lib.wd_silu_bwd, (pre2.data_ptr(), de2.data_ptr(), B * ted, dpre2.data_ptr()), "emb SiLU:bwd"))
        if rows is not None:
            # the slot of every sample's writer in the row list (-1: not being fitted), then the scatter into the compact buffer
            R = len(rows)
            rows_c = (C.c_int * R)(*rows)
            slots = torch.empty((B,), dtype=torch.int64, device=self.device)
            P.row_grad = torch.zeros((R, ted), dtype=torch.float32, device=self.device)
            P.keep += [rows_c, slots]
            bops.append((lib.wd_row_slots, (y_bwd.data_ptr(), B, rows_c, R, m.num_classes, slots.data_ptr()), "label_emb:row slots"))
            bops.append((lib.wd_embedding_bwd, (slots.data_ptr(), 1, B, dpre2.data_ptr(), ted, R, ted, P.row_grad.data_ptr(), 0),
                         "label_emb:bwd(rows)"))
            return
        if y_bwd is not None:
            dl = self._pgrad(m.label_emb.weight)
            bops.append((lib.wd_embedding_bwd, (y_bwd.data_ptr(), 1, B, dpre2.data_ptr(), ted, m.num_classes, ted, dl.data_ptr(),
                                                self._pacc(dl)), "label_emb:bwd"))
        de1 = self._f32(P, B, ted)
        self._bwd_linear(P, "time_embed.2", dpre2, B, ted, 1,
                         [linear_seg(e1, ted, 1, "B:te2.w", self._pgrad(m.time_embed[2].weight), de1, B)],
                         bias=[self._pgrad(m.time_embed[2].bias)])
        dpre1 = self._f32(P, B, ted)
        bops.append((lib.wd_silu_bwd, (pre1.data_ptr(), de1.data_ptr(), B * ted, dpre1.data_ptr()), "time SiLU:bwd"))
        self._bwd_linear(P, "time_embed.0", dpre1, B, ted, 1,
                         [BwdSeg(te, mc, 1, 1, wgrad=self._pgrad(m.time_embed[0].weight))], bias=[self._pgrad(m.time_embed[0].bias)])

    def _cond_bwd(self, P, groups, L):
        """Appends the conditioning path's backward to ``P.bwd``: d(K | V) through the K/V projections of every cross-attention
        into d(context), then per token group the word encoder's attention, q|k|v projection and embedding table."""
        m, lib, B, bops = self.model, self.lib, self._B, P.bwd
        cd = m.context_dim
        kv_w = self._pgroup([w for at in self._kv_mods for w in (at.to_k.weight, at.to_v.weight)])
        dctx = self._f32(P, B * L, cd)
        self._bwd_linear(P, "cross.kv", self._bs.dkv, B * L, self.kv_total, L,
                         [linear_seg(P.ctx_pl, cd, L, "B:kv.w", kv_w, dctx, B * L)])
        we = m.word_emb
        at = we.attention
        qkv_w = self._pgroup([at.linear_query.weight, at.linear_key.weight, at.linear_value.weight])
        qkv_b = self._pgroup([at.linear_query.bias, at.linear_key.bias, at.linear_value.bias])
        dtab = self._pgrad(we.embedding.weight)
        for (ids, n_tok, row0, i64, e, qkv) in groups:
            if n_tok == L:
                dgrp = dctx
            else:  # this group's rows of every sample, made contiguous
                dgrp = self._f32(P, B * n_tok, cd)
                bops.append((lib.wd_copy2d, (dgrp.data_ptr(), 4 * n_tok * cd, dctx.data_ptr() + 4 * row0 * cd, 4 * L * cd,
                                             4 * n_tok * cd, B), "d(context):group rows"))
            dqkv = self._f32(P, B * n_tok, 3 * cd)
            self._attn_bwd(P, "word_emb.attention:bwd", qkv.data_ptr(), 3 * cd, qkv.data_ptr() + 4 * cd, 3 * cd,
                           qkv.data_ptr() + 8 * cd, 3 * cd, dgrp, 1, n_tok, n_tok, cd, 1.0, dqkv.data_ptr(), 3 * cd,
                           dqkv.data_ptr() + 4 * cd, 3 * cd)
            de = self._f32(P, B * n_tok, cd)
            self._bwd_linear(P, "word_emb.qkv", dqkv, B * n_tok, 3 * cd, n_tok,
                             [linear_seg(e, cd, n_tok, "B:we.qkv.w", qkv_w, de, B * n_tok)], bias=[qkv_b])
            bops.append((lib.wd_embedding_bwd, (ids.data_ptr(), i64, B * n_tok, de.data_ptr(), cd, we.embedding.weight.shape[0], cd,
                                                dtab.data_ptr(), self._pacc(dtab)), "word_emb.embedding:bwd"))

    def _arena_segments(self, P) -> List[tuple]:
        """[(bwd_begin, bwd_end, arena_begin, arena_end)] per bucket of ``P.bwd_cuts``: the arena prefix that is final at each cut
        is the longest prefix (in carve order) of buffers whose last writer is a closure <= the cut's (buffers never written by
        this plan - dead heads - count as final)."""
        segments = []
        lo_op, lo_ar = 0, 0
        for (op_end, closure) in P.bwd_cuts:
            hi_ar = lo_ar
            for (ptr, off, n) in self._carve_order:
                if off < lo_ar:
                    continue
                if self._bs.done_at.get(ptr, 0) > closure:
                    break
                hi_ar = off + n
            segments.append((lo_op, op_end, lo_ar, hi_ar))
            lo_op, lo_ar = op_end, hi_ar
        return segments + [(lo_op, len(P.bwd), lo_ar, self._arena_used)]

    # ------------------------------------------------------------------------------------------ run
    def forward_train(self, x, t, context, y, phosc=None, writer_keep=None):
        """Training forward: keeps every intermediate for ``backward``.  Returns the plan's output buffer (no copy).
        writer_keep: bool / uint8 [B] or False (``UNetEngine.load_keep``) - the writer term per sample, in the forward and in
        label_emb's gradient."""
        self.refresh_weights()
        B, _, H, W = x.shape
        if context is None:
            raise NotImplementedError("context=None")
        self.check_ids(context, y, phosc)
        if writer_keep is not None and writer_keep is not False:
            writer_keep = check_writer_keep(writer_keep, B)
        P = self.plan_train(B, H, W, context.shape[1], 0 if phosc is None else phosc.shape[1],
                            **(dict(label_drop="mask") if writer_keep is not None else {}))
        self.load_inputs(P, x, t, context, y, phosc, check=False)
        if writer_keep is not None:
            self.load_keep(P, writer_keep)
        if P.dropouts:
            P.set_dropout_seed(self.dropout_seed)
            P.set_row_base(self.dropout_row_base)
            self.dropout_row_base += B
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self.claim_forward(P)
        P.run_step(stream)
        return P.out

    # One training shape is live per engine (plan_train), and a plan keeps the intermediates of ONE forward.  A forward is
    # therefore identified by (plan, serial); whoever is about to overwrite a plan's intermediates says so first.
    def claim_forward(self, P: TrainPlan) -> tuple:
        """Called by whoever is about to run ``P.step`` (``forward_train``, ``TrainStep``): the plan becomes the one ``backward``
        differentiates and every earlier forward's identity goes stale.  Returns the new identity (``last_forward``)."""
        self._serial += 1
        P.serial = self._serial
        self._live = P
        return (P, P.serial)

    def last_forward(self) -> Optional[tuple]:
        """The identity of the latest training forward, (plan, serial), for ``backward(forward=...)``; None before the first."""
        return None if self._live is None else (self._live, self._live.serial)

    def holds_plan(self, P: Optional[TrainPlan]) -> bool:
        """Whether ``P`` is still a plan of this engine.  False once a plan of another key was built (or the precision changed):
        the shared scratch ``P``'s launches point into is released then, so ``P`` must never run again."""
        return P is not None and any(q is P for q in self._tplans.values())

    def _check_forward(self, forward: tuple) -> TrainPlan:
        P, serial = forward
        what = "a later forward on this model overwrote the activations this backward needs"
        if not self.holds_plan(P):
            what += " (it ran at another shape or precision, which released this forward's training plan)"
        elif self._live is P and P.serial == serial:
            return P
        raise RuntimeError(what + ": the HIP training path keeps the intermediates of one forward per model.  Run one forward per "
                           "backward, and any other forward in between under torch.no_grad() or model.eval() (the inference "
                           "engine, which leaves the training plan alone)")

    def backward(self, dout: torch.Tensor, assign: bool = True, forward: Optional[tuple] = None):
        """Runs the backward list for d loss / d out (NCHW) and points ``param.grad`` at the gradient buffers (adding to
        a ``.grad`` the caller kept, like autograd's accumulation).

        forward: the identity of the forward to differentiate, as ``last_forward()`` returned it right after that forward (the
        autograd node of ``model(...)`` passes its own).  Raises a RuntimeError, before anything is copied, launched or assigned,
        when that forward's plan was released or a later forward overwrote its intermediates.  None: the latest forward.

        A second backward through one forward (``loss.backward(retain_graph=True)`` twice) is valid and repeats the first bit for
        bit, so with ``assign`` the gradients end up exactly doubled, as autograd's accumulation would leave them: the backward
        list never writes a buffer the forward saved (operand planes, pre-activations, GroupNorm statistics, K | V, attention
        outputs are only read).  Every buffer it writes is its own - ``P.dout``, the activation gradients, whose first writer in list
        order overwrites and later ones add (``_gacc`` / ``Dx.acc``), the parameter gradients (``_pacc``, the same rule) - or shared
        scratch (``dpl``, ``doutT``, ``xT``, ``colpart``, ``attn_bwd``, the workspace) that is refilled before each read; the dropout
        masks are re-derived from the plan's seed and device row base, which only a forward changes."""
        if forward is not None:
            P = self._check_forward(forward)
        elif not self.holds_plan(self._live):
            raise RuntimeError("backward without a training forward: forward_train has not run on this engine, or the plan of "
                               "its latest forward was released since (a plan of another key, a change of precision)")
        else:
            P = self._live
        kept = []
        if assign:
            for k, p in self._params.items():
                if p.grad is not None:
                    # the caller did not reset this gradient to None (zero_grad(set_to_none=False) / accumulation)
                    kept.append((k, p.grad.clone() if p.grad.data_ptr() == self._grad[k].data_ptr() else p.grad))
        P.dout.copy_(dout, non_blocking=True)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        P.run_bwd(stream)
        if assign:
            for k, old in kept:
                self._grad[k].add_(old)
            self.assign_grads()

    def assign_grads(self):
        for k, p in self._params.items():
            p.grad = self._grad[k]

    def grads(self) -> Dict[str, torch.Tensor]:
        names = {id(p): n for n, p in self.model.named_parameters()}
        return {names[k]: g for k, g in self._grad.items()}
