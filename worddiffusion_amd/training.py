"""The body of the reference's training loop (``train.py:277-294``) as a handful of device launches:

    t = diffusion.sample_timesteps(B); x_t, noise = diffusion.noise_images(latents, t)        train.py:281-282
    predicted_noise = model(x_t, ..., timesteps=t, context=text_features, y=labels)            train.py:287
    loss = mse(noise, predicted_noise); optimizer.zero_grad(); loss.backward()                 train.py:289-291
    optimizer.step(); ema.step_ema(ema_model, model)                                           train.py:293-294

``TrainStep`` runs noise_images + forward + loss + backward as ONE hipGraph, then one multi-tensor AdamW+EMA launch and one
weight-repack launch.  Data-parallel (world > 1): the backward list is cut into a few segments (``WDIFF_GRAD_BUCKETS``, default 3)
after each of which a PREFIX of the flat gradient arena is final - the gradients of the layers nearest the output, which the
backward pass finishes first; every segment is its own hipGraph and the all-reduce of its prefix (RCCL over xGMI) runs on a
second stream while the next segment computes, so only the last bucket's collective is exposed.  The same arithmetic is
reachable piecewise through the reference's own call surface (``model(...)``, ``loss.backward()``, ``FusedAdamW.step``);
this class only removes the per-step host work.

Gradient accumulation (``accumulate=A``): an optimiser step happens on every A-th call.  A call that does not end its group runs
the same captured graph and then adds the gradient arena into a second arena-sized buffer (``wd_grad_accumulate``; the first call
of a group overwrites it) - no collective, no ``param.grad`` assignment, no optimiser step, no weight repack.  The last call folds
the buffer back into the arena, scales by 1 / A (1 / (A * world) after the all-reduce) and goes on as a plain step, so
``eng.grads()`` / ``param.grad`` then hold the MEAN gradient over the group, before any clipping, and the AdamW table keeps its
pointers.  Data-parallel: collectives are issued on the last call only; in the bucketed form the fold of prefix [a0, a1) is queued
on the compute stream behind segment j and in front of the event its all-reduce waits on, so the overlap is the plain step's.

Keying invariant: ``step_index`` counts CALLS, with or without accumulation, and the eps rows, the dropout masks and the writer
dropout (``label_dropout``) of call c are keyed by the global row ``(c * world + rank) * B + b``.  So A calls of B rows draw
exactly what one call of A * B rows draws.

A partial group carries over from one call (and one ``train_epoch``) to the next - the buffer and ``micro_index`` belong to this
object -, but neither is in a checkpoint: save at ``micro_index == 0``.

Global-norm clipping belongs to the optimiser handed in (``FusedAdamW(max_grad_norm=...)``); ``last_grad_norm`` is its
``grad_norm``, the norm of the mean gradient of the last optimiser step.

Weighted loss (``loss_weights`` / ``loss_bins`` / ``loss_mask``; DESIGN.md "Weighted training loss"): the step's loss launch becomes
``wd_weighted_mse_loss`` - loss = mean_b w[t_b] * sum_i m_bi (pred - eps)_bi^2 / sum_i m_bi -, which also writes the per-sample
losses and adds them to a per-timestep histogram, inside the captured body.  Accumulation, clipping and data-parallel need no
change: the gradient is still d loss / d pred of a per-rank mean over B, so the arena holds what it always held.  A step built
without the new arguments, and never handed a mask, launches ``wd_mse_loss`` as before and allocates nothing new.

Fitting new writers (an ``optim.RowAdamW`` as the optimiser; DESIGN.md "Fitting new writers"): the trunk is frozen and only the
optimiser's rows of ``label_emb`` train.  The captured body is noise -> forward -> loss -> the frozen-trunk backward
(``plan_train(rows=...)``: no weight gradient, no ResBlock dropout), whose last launch writes the optimiser's compact ``row_grad``;
then ``opt.step()``.  Nothing assigns ``param.grad`` (frozen parameters keep ``grad is None``) and there is no all-reduce.  The loss
launch is the same, so the weighted-loss arguments, ``t=`` / ``noise=`` / ``check=`` and the keying invariant work unchanged.
Samples whose writer is not among the rows are legal: they cost a forward and add no gradient.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _native as N
from .dropout import check_p
from .optim import FusedAdamW, RowAdamW, check_loss_weights, check_timesteps, expand_loss_mask


class TrainStep:
    def __init__(self, model, diffusion, optimizer: FusedAdamW, seed: int = 0, use_graph: bool = True,
                 process_group=None, bucketed: Optional[bool] = None, accumulate: int = 1, loss_weights=None,
                 snr_gamma: float = 5.0, loss_bins: int = 0, label_dropout: float = 0.0):
        """``bucketed``: run the backward pass in segments with the gradient all-reduce of each segment's arena prefix
        overlapped with the next segment (default: whenever world > 1; ``True`` at world 1 only cuts the graph - tests).
        ``accumulate``: calls per optimiser step (module docstring); 1 is the plain step, launch for launch.
        ``loss_weights``: ``None``, ``"min_snr"`` (``diffusion.min_snr_weights(snr_gamma)``) or a float tensor [noise_steps],
        finite and >= 0: the weight of a sample drawn at timestep t; the returned loss is the weighted one.
        ``loss_bins``: > 0 keeps a histogram of the UNWEIGHTED per-sample losses over that many equal timestep ranges
        (``loss_by_timestep()``), updated on the device by the loss launch itself.
        ``label_dropout``: p in [0, 1) - every sample runs without its writer term with probability p (the training half of
        writer-free guidance), drawn on the device inside the captured body under the keying invariant of the module docstring;
        ``last_writer_keep`` holds the decisions of the last call.  0 is the step without the argument, launch for launch."""
        self.label_dropout = check_p(label_dropout)
        self.frozen = isinstance(optimizer, RowAdamW)
        if self.frozen:  # refused before anything is launched
            if accumulate != 1:
                raise ValueError("fitting writer rows (RowAdamW) does not accumulate: accumulate must be 1")
            if self.label_dropout > 0:
                raise ValueError("a row being fitted must keep its writer term: label_dropout must be 0 with a RowAdamW")
            if bucketed:
                raise ValueError("fitting writer rows (RowAdamW) has no gradient buckets: bucketed must not be True")
            if getattr(getattr(model, "label_emb", None), "weight", None) is not optimizer.table:
                raise ValueError("the RowAdamW's table is not this model's label_emb.weight")
        if int(accumulate) != accumulate or accumulate < 1:
            raise ValueError(f"accumulate must be an integer >= 1, got {accumulate!r}")
        if isinstance(loss_bins, bool) or int(loss_bins) != loss_bins or loss_bins < 0:
            raise ValueError(f"loss_bins must be an integer >= 0, got {loss_bins!r}")
        if loss_weights is None:
            self._wtab_host = None
        elif isinstance(loss_weights, str):
            if loss_weights != "min_snr":
                raise ValueError(f"loss_weights must be None, 'min_snr' or a float tensor [noise_steps], not {loss_weights!r}")
            self._wtab_host = check_loss_weights(diffusion.min_snr_weights(snr_gamma), diffusion.noise_steps)
        else:
            self._wtab_host = check_loss_weights(loss_weights, diffusion.noise_steps)
        self.loss_bins = int(loss_bins)
        self._weighted = self._wtab_host is not None or self.loss_bins > 0  # the loss launch is wd_weighted_mse_loss even unmasked
        self._wtab = self._hist = self._sample_loss = self._wscratch = self._mask = None  # made by the first call that needs them
        self._mgraph = self._mseg_graphs = None  # the captured bodies of masked calls (``_graph`` / ``_seg_graphs``: unmasked)
        self.model, self.diffusion, self.opt = model, diffusion, optimizer
        self.seed, self.use_graph = seed, use_graph
        self.accumulate = int(accumulate)
        self.micro_index = 0      # position of the next call inside its group, 0 .. accumulate - 1
        self.optimizer_steps = 0  # optimiser steps taken (step_index counts calls)
        self._acc = None          # the accumulation buffer, arena-sized, allocated by the first call that needs it
        self._bucketed_arg = bucketed
        self.lib = N.lib()
        self.eng = model.train_engine
        self.step_index = 0
        self._key = None
        self._P = None
        self._graph = None
        self.pg = process_group
        self.world, self.rank = 1, 0
        if process_group is not None or (torch.distributed.is_available() and torch.distributed.is_initialized()):
            self.world = torch.distributed.get_world_size(process_group)
            self.rank = torch.distributed.get_rank(process_group)
        if self.frozen and self.world > 1:
            raise ValueError("fitting writer rows (RowAdamW) is single-process: world size must be 1")
        # data-parallel ranks must not draw the same (eps, t): the noise rows are keyed by the GLOBAL row of the step
        # (``(step * world + rank) * B + b``, so world ranks of batch B draw what one process of batch world*B would), and the
        # timesteps come from a per-rank host generator (a single process keeps the reference's global host RNG, train.py:281)
        self._tgen = torch.Generator().manual_seed((int(seed) * 1000003 + self.rank) & 0x7FFFFFFFFFFFFFFF) if self.world > 1 \
            else None

    def _prepare(self, B, H, W, L, dev, phosc_len=0):
        eng = self.eng
        eng.refresh_weights()
        if self.frozen:
            P = eng.plan_train(B, H, W, L, phosc_len, rows=self.opt.rows)
            self.opt.bind_grad(P.row_grad)  # the plan's last launch writes the optimiser's compact gradient
        else:
            P = eng.plan_train(B, H, W, L, phosc_len, **(dict(label_drop=self.label_dropout) if self.label_dropout > 0 else {}))
        ah = self.diffusion.alpha_hat.cpu()
        self._sa, self._sb = torch.sqrt(ah).to(dev).contiguous(), torch.sqrt(1 - ah).to(dev).contiguous()
        self._x0 = torch.zeros_like(P.x_in)
        self._eps = torch.zeros_like(P.x_in)
        self._loss = torch.zeros(1, dtype=torch.float32, device=dev)
        self._scratch = torch.zeros(1024, dtype=torch.float64, device=dev)
        self._P = P
        self._stream = torch.cuda.Stream(device=dev)
        self._comm = torch.cuda.Stream(device=dev)
        for g in [self._graph, self._mgraph] + list(getattr(self, "_seg_graphs", []) or []) + list(self._mseg_graphs or []):
            if g is not None:
                self.lib.wd_graph_destroy(g)
        self._graph = self._mgraph = None
        self._seg_graphs = self._mseg_graphs = None
        self._sample_loss = self._wscratch = self._mask = None  # sized by the batch (the histogram and the table are not)
        self.bucketed = (self.world > 1) if self._bucketed_arg is None else bool(self._bucketed_arg)
        self.segments = list(getattr(P, "bwd_segments", [])) if self.bucketed else []
        if len(self.segments) <= 1:
            self.segments = []

    def _ensure_weighted(self, masked: bool):
        """The buffers of the weighted loss launch, allocated by the first call that runs it (never by a plain step)."""
        P = self._P
        dev, B = P.x_in.device, P.x_in.shape[0]
        if self._sample_loss is None:
            for name, buf in (("out", P.out), ("dout", P.dout), ("eps", self._eps)):  # [B][C*h*w] rows, as the flat MSE assumes
                if tuple(buf.shape) != tuple(P.x_in.shape) or not buf.is_contiguous():
                    raise N.NativeError(f"the training plan's {name} does not share the layout of its input")
            self._sample_loss = torch.zeros(B, dtype=torch.float32, device=dev)
            self._wscratch = torch.zeros(2 * B, dtype=torch.float64, device=dev)
        if self._wtab_host is not None and (self._wtab is None or self._wtab.device != dev):
            self._wtab = self._wtab_host.to(dev)
        if self.loss_bins and (self._hist is None or self._hist.device != dev):
            self._hist = torch.zeros(self.loss_bins, 2, dtype=torch.float64, device=dev)
        if masked and self._mask is None:
            self._mask = torch.zeros(B, P.x_in[0].numel(), dtype=torch.float32, device=dev)

    def _body(self, st, seg: Optional[int] = None, masked: bool = False):
        """The whole step body (seg None), or segment ``seg`` of it: segment 0 = noise + forward + loss + the first part of the
        backward list, the others = the following parts.  ``masked``: the loss launch reads the step's mask buffer."""
        lib, P = self.lib, self._P
        if seg is None or seg == 0:
            n = P.x_in[0].numel()
            B = P.x_in.shape[0]
            N.check(lib.wd_noise_images(self._x0.data_ptr(), self._eps.data_ptr(), P.t_in.data_ptr(), self._sa.data_ptr(),
                                        self._sb.data_ptr(), B, n, P.x_in.data_ptr(), st), "wd_noise_images")
            P.run_step(st)
            if self._weighted or masked:
                N.check(lib.wd_weighted_mse_loss(P.out.data_ptr(), self._eps.data_ptr(), self._mask.data_ptr() if masked else None,
                                                 B, n, P.t_in.data_ptr(), None if self._wtab is None else self._wtab.data_ptr(),
                                                 self.diffusion.noise_steps, P.dout.data_ptr(), self._loss.data_ptr(),
                                                 self._sample_loss.data_ptr(), None if self._hist is None else self._hist.data_ptr(),
                                                 self.loss_bins, self._wscratch.data_ptr(), st), "wd_weighted_mse_loss")
            else:
                N.check(lib.wd_mse_loss(P.out.data_ptr(), self._eps.data_ptr(), P.out.numel(), P.dout.data_ptr(),
                                        self._loss.data_ptr(), self._scratch.data_ptr(), 1024, st), "wd_mse_loss")
        if seg is None:
            P.run_bwd(st)
        else:
            b0, b1, _, _ = self.segments[seg]
            P.run_bwd(st, b0, b1)

    def _capture(self, st, seg=None, masked=False):
        lib = self.lib
        N.check(lib.wd_graph_begin(st), "wd_graph_begin")
        g = C.c_void_p()
        try:
            self._body(st, seg, masked)
        finally:
            rc = lib.wd_graph_end(st, C.byref(g))
        N.check(rc, "wd_graph_end")
        return g

    def _accumulate(self, st, a0, a1, fold: bool):
        """fold False: acc[a0:a1] (+)= arena[a0:a1] (the first call of a group overwrites: the buffer is never cleared);
        fold True: arena[a0:a1] = s * (arena[a0:a1] + acc[a0:a1]), s = 1 / accumulate in a single process and 1 in front of an
        all-reduce (the sum over ranks is scaled once, by 1 / (accumulate * world))."""
        arena = self.eng.grad_arena()
        if self._acc is None or self._acc.numel() != arena.numel():
            if self.micro_index != 0:
                raise RuntimeError("the gradient arena changed size inside an accumulation group")
            self._acc = torch.empty_like(arena)
        if a1 <= a0:
            return
        dst, src = (arena, self._acc) if fold else (self._acc, arena)
        scale = 1.0 / self.accumulate if fold and self.world == 1 else 1.0
        N.check(self.lib.wd_grad_accumulate(dst[a0:a1].data_ptr(), src[a0:a1].data_ptr(), a1 - a0,
                                            0 if fold or self.micro_index else 1, scale, st), "wd_grad_accumulate")

    def _run_bucketed(self, st, final: bool = True, masked: bool = False):
        """Backward in segments; after segment j the arena prefix [a0, a1) is final: its all-reduce goes to the comm stream
        behind an event, the next segment runs meanwhile.  Returns after queueing everything; the compute stream waits for
        the collectives before the optimiser.  ``final`` False (a call inside an accumulation group): the segments only."""
        lib = self.lib
        arena = self.eng.grad_arena()
        graphs = None
        if self.use_graph:  # one list of segment graphs per variant of the body; only segment 0, which holds the loss, differs
            if (self._mseg_graphs if masked else self._seg_graphs) is None:
                made = [self._capture(st, j, masked) for j in range(len(self.segments))]
                if masked:
                    self._mseg_graphs = made
                else:
                    self._seg_graphs = made
            graphs = self._mseg_graphs if masked else self._seg_graphs
        for j, (_, _, a0, a1) in enumerate(self.segments):
            if self.use_graph:
                N.check(lib.wd_graph_launch(graphs[j], st), "wd_graph_launch")
            else:
                self._body(st, j, masked)
            if final and self.accumulate > 1:
                self._accumulate(st, a0, a1, fold=True)  # in front of the event: the collective sums whole groups
            if final and self.world > 1 and a1 > a0:
                ev = torch.cuda.Event()
                ev.record(self._stream)
                self._comm.wait_event(ev)
                with torch.cuda.stream(self._comm):
                    torch.distributed.all_reduce(arena[a0:a1], group=self.pg)  # RCCL over xGMI (gloo in the one-GPU tests)
        if final and self.world > 1:
            self._stream.wait_stream(self._comm)
            arena.mul_(1.0 / (self.accumulate * self.world))

    def __call__(self, latents: torch.Tensor, text_features: torch.Tensor, labels: Optional[torch.Tensor],
                 t: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
                 phoscLabels: Optional[torch.Tensor] = None, check: bool = True,
                 loss_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One optimisation step on a batch of latents [B, C, H, W]; returns the loss as a device tensor [1] (the
        reference's ``loss.item()`` per step, train.py:295, is the caller's choice).  With ``accumulate > 1`` the batch is one
        micro-batch of its group, the loss is this micro-batch's, and the optimiser steps on the group's last call.

        ``loss_mask``: a weight in [0, 1] per latent cell, of shape [h, w], [B, 1, h, w] or [B, C, h, w] (the known-region
        convention); sample b's loss is then the mask-weighted mean over its cells, and a sample whose mask is all zero adds
        nothing.  The mask is copied into a buffer of the step before the graph runs.  Masked and unmasked calls are two captured
        bodies, each kept once it exists.  ``check`` also covers the mask's values and a host ``t`` (every value in
        [0, noise_steps): the loss launch indexes its tables with it); a mask on the device costs one small synchronisation
        there, so a loader that has checked its host tensors passes ``check=False``."""
        if not latents.is_cuda:
            raise N.NativeError("TrainStep runs on the GPU only (no CPU fallback)")
        dev = latents.device
        B, _, H, W = latents.shape
        phosc_len = 0 if phoscLabels is None else phoscLabels.shape[1]
        key = (B, H, W, text_features.shape[1], phosc_len, str(dev))
        # the engine keeps one training plan: anything else that trains this model at another shape in between (model(...) under
        # autograd, a second TrainStep) released the scratch this step's plan and captured graphs point into.  Then the plan is
        # built and captured again; nothing of the old one runs (``_prepare`` only destroys its graphs, a host-side call).
        if key != self._key or not self.eng.holds_plan(self._P):
            self._prepare(B, H, W, text_features.shape[1], dev, phosc_len)
            self._key = key
        lib, P = self.lib, self._P
        self.eng.claim_forward(P)  # this call overwrites the plan's intermediates: a pending backward of model(...) is refused
        if check:  # out-of-range ids raise here instead of faulting a kernel (device tensors: one small sync; a loader that has
            self.eng.check_ids(text_features, labels, phoscLabels)  # checked its host tensors passes check=False)
            if t is not None and not t.is_cuda:
                check_timesteps(t, B, self.diffusion.noise_steps)
        masked = loss_mask is not None
        if masked:
            loss_mask = expand_loss_mask(loss_mask, latents.shape, check_values=check)
        if masked or self._weighted:
            self._ensure_weighted(masked)
        if t is None:
            if self._tgen is None:
                t = self.diffusion.sample_timesteps(B)  # host RNG like the reference (train.py:281)
            else:
                t = torch.randint(low=1, high=self.diffusion.noise_steps, size=(B,), generator=self._tgen)
        # the legacy default stream cannot be captured: the step runs on its own stream, ordered after the caller's work
        # and before whatever the caller enqueues next
        cur = torch.cuda.current_stream(dev)
        self._stream.wait_stream(cur)
        with torch.cuda.stream(self._stream):
            st = self._stream.cuda_stream
            P.t_in.copy_(t, non_blocking=True)
            # training dropout: masks keyed like the eps rows below - (seed, global row of the step) -, the row read on the device
            # so that the captured step draws new masks every time it is replayed
            P.set_dropout_seed(self.seed)
            P.set_row_base((self.step_index * self.world + self.rank) * B)
            P.ctx_in.copy_(text_features, non_blocking=True)
            if phoscLabels is not None:  # UNetModelPhosc: PHOSC vector appended to the context (unetPhosc.py:1119-1131)
                P.phosc_in.copy_(phoscLabels.to(torch.int32) if phoscLabels.dtype != torch.int32 else phoscLabels,
                                 non_blocking=True)
            if labels is not None:
                P.y_in.copy_(labels, non_blocking=True)
            self._x0.copy_(latents, non_blocking=True)
            if masked:
                self._mask.copy_(loss_mask, non_blocking=True)
            if noise is not None:
                self._eps.copy_(noise, non_blocking=True)
            else:
                N.check(lib.wd_randn(self._eps.data_ptr(), B, self._eps[0].numel(), self.seed,
                                     (self.step_index * self.world + self.rank) * B, 2, st), "wd_randn")
            final = self.micro_index == self.accumulate - 1  # this call ends its group: the optimiser steps
            if self.segments:
                self._run_bucketed(st, final, masked)
            else:
                if self.use_graph:
                    if masked and self._mgraph is None:
                        self._mgraph = self._capture(st, None, True)
                    elif not masked and self._graph is None:
                        self._graph = self._capture(st)
                    N.check(lib.wd_graph_launch(self._mgraph if masked else self._graph, st), "wd_graph_launch")
                else:
                    self._body(st, None, masked)
                if final and self.accumulate > 1:
                    self._accumulate(st, 0, self.eng.grad_arena().numel(), fold=True)
                if final and self.world > 1:
                    arena = self.eng.grad_arena()
                    torch.distributed.all_reduce(arena, group=self.pg)  # one all-reduce of the whole arena (WDIFF_GRAD_BUCKETS=1)
                    arena.mul_(1.0 / (self.accumulate * self.world))
            if final:
                if not self.frozen:
                    self.eng.assign_grads()
                self.opt.step()
                self.eng.refresh_weights()
            else:
                self._accumulate(st, 0, self.eng.grad_arena().numel(), fold=False)
        cur.wait_stream(self._stream)
        for tns in (latents, text_features, labels, noise, loss_mask):
            if tns is not None and tns.is_cuda:
                tns.record_stream(self._stream)
        self.step_index += 1
        if final:
            self.micro_index = 0
            self.optimizer_steps += 1
        else:
            self.micro_index += 1
        return self._loss

    @property
    def last_grad_norm(self) -> torch.Tensor:
        """The optimiser's ``grad_norm``: device fp32 [1], the global norm of the (mean) gradient of the last optimiser step,
        before clipping (``FusedAdamW(max_grad_norm=...)``; zero while clipping is off)."""
        return self.opt.grad_norm

    @property
    def last_writer_keep(self) -> torch.Tensor:
        """Device uint8 [B]: 1 where the sample of the last call kept its writer term, written by the step itself; nothing
        synchronises.  Only a step built with ``label_dropout > 0`` draws it."""
        if not self.label_dropout or self._key is None:
            raise RuntimeError("last_writer_keep: no call has drawn a writer dropout (TrainStep(label_dropout > 0))")
        return self._P.writer_keep

    @property
    def last_sample_losses(self) -> torch.Tensor:
        """Device fp32 [B]: the UNWEIGHTED (masked) mean squared error of every sample of the last call, written by the loss launch;
        nothing synchronises.  Only the weighted loss launch computes it (``loss_weights``, ``loss_bins`` or a ``loss_mask``)."""
        if self._sample_loss is None:
            raise RuntimeError("last_sample_losses: no call has run the weighted loss (loss_weights, loss_bins or a loss_mask)")
        return self._sample_loss

    def _bin_edges(self):
        T, nb = self.diffusion.noise_steps, self.loss_bins
        return [-((-k * T) // nb) for k in range(nb)] + [T]  # bin k holds the t with (t * nb) // T == k: from ceil(k T / nb) on

    def loss_by_timestep(self):
        """The histogram ``loss_bins`` asked for, as numpy arrays: ``edges`` int64 [loss_bins + 1] (bin k holds the timesteps
        edges[k] <= t < edges[k + 1]), ``mean`` float64 [loss_bins] (the mean unweighted per-sample loss of the calls since the
        last reset; NaN for a bin no sample fell in) and ``count`` int64 [loss_bins].  Synchronises once, here and nowhere else."""
        import numpy as np
        if not self.loss_bins:
            raise RuntimeError("loss_by_timestep needs TrainStep(loss_bins > 0)")
        if self._hist is None:
            h = np.zeros((self.loss_bins, 2))
        else:
            h = self._hist.cpu().numpy()  # (the one synchronisation; ordered after the step, which the caller's stream waits for)
        count = h[:, 1].astype(np.int64)
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = np.where(count > 0, h[:, 0] / h[:, 1], np.nan)
        return dict(edges=np.asarray(self._bin_edges(), dtype=np.int64), mean=mean, count=count)

    def reset_loss_by_timestep(self) -> None:
        """Empties the histogram (a device memset queued behind the last step; no synchronisation)."""
        if not self.loss_bins:
            raise RuntimeError("reset_loss_by_timestep needs TrainStep(loss_bins > 0)")
        if self._hist is not None:
            self._hist.zero_()
