"""Optimiser side of the reference's training step (``train.py:289-294``): ``mse_loss`` and ``FusedAdamW`` - one HIP
launch updates every parameter (and the EMA copy) instead of the reference's ~260 x 3 elementwise launches per step for
``AdamW.step`` + ``EMA.step_ema``.  Gradients come from the caller (``param.grad``); the backward kernels of the UNet are
the next row of the plan."""
from __future__ import annotations

from typing import Optional

import torch

from . import _native as N


def mse_loss(pred: torch.Tensor, target: torch.Tensor, want_grad: bool = True):
    """nn.MSELoss()(target, pred) (train.py:289) -> (loss [1] device tensor, d loss / d pred or None)."""
    if not pred.is_cuda:
        raise N.NativeError("mse_loss runs on the GPU only (no CPU fallback)")
    lib = N.lib()
    pred, target = pred.contiguous().float(), target.contiguous().float()
    n = pred.numel()
    grad = torch.empty_like(pred) if want_grad else None
    loss = torch.empty(1, dtype=torch.float32, device=pred.device)
    scratch = torch.empty(1024, dtype=torch.float64, device=pred.device)
    st = torch.cuda.current_stream(pred.device).cuda_stream
    N.check(lib.wd_mse_loss(pred.data_ptr(), target.data_ptr(), n, grad.data_ptr() if want_grad else None, loss.data_ptr(),
                            scratch.data_ptr(), 1024, st), "wd_mse_loss")
    return loss, grad


def expand_loss_mask(mask, shape, check_values: bool = True) -> torch.Tensor:
    """A loss mask under the known-region rules (``Diffusion._known_setup``): a float (or bool) tensor of shape ``[h, w]``,
    ``[B, 1, h, w]`` or ``[B, C, h, w]`` for predictions of ``shape = (B, C, h, w)``, values in [0, 1] -> fp32 ``[B, C*h*w]`` on the
    mask's own device.  Host arithmetic only (``check_values`` on a device tensor costs one small synchronisation)."""
    shape = tuple(int(v) for v in shape)
    if len(shape) != 4:
        raise ValueError(f"a loss mask needs predictions of shape [B, C, h, w], got {list(shape)}")
    B, C, h, w = shape
    mask = torch.as_tensor(mask)
    if mask.dtype == torch.bool:
        mask = mask.to(torch.float32)
    if not mask.is_floating_point() or tuple(mask.shape) not in ((h, w), (B, 1, h, w), shape):
        raise ValueError(f"loss_mask must be a float tensor [{h}, {w}], [{B}, 1, {h}, {w}] or {list(shape)}, "
                         f"got {mask.dtype} {tuple(mask.shape)}")
    mask = mask.detach().to(torch.float32)
    if check_values and not bool(((mask >= 0) & (mask <= 1)).all()):  # (NaN fails both comparisons)
        raise ValueError("loss_mask values must lie in [0, 1]")
    return mask.expand(B, C, h, w).reshape(B, -1).contiguous()


def check_loss_weights(weights, noise_steps: int) -> torch.Tensor:
    """A per-timestep weight table: a float tensor ``[noise_steps]``, every value finite and >= 0 -> fp32 on the host."""
    w = torch.as_tensor(weights)
    if not w.is_floating_point() or tuple(w.shape) != (int(noise_steps),):
        raise ValueError(f"loss weights must be a float tensor [{int(noise_steps)}], got {w.dtype} {tuple(w.shape)}")
    w = w.detach().to(torch.float32).cpu().contiguous()
    if not bool((torch.isfinite(w) & (w >= 0)).all()):
        raise ValueError("loss weights must be finite and >= 0")
    return w


def check_timesteps(t, batch: int, noise_steps: int) -> torch.Tensor:
    """Timesteps that index a per-timestep table: an integer tensor ``[batch]`` with every value in [0, noise_steps)."""
    t = torch.as_tensor(t)
    if t.is_floating_point() or t.dtype == torch.bool or tuple(t.shape) != (int(batch),):
        raise ValueError(f"t must be an integer tensor [{int(batch)}], got {t.dtype} {tuple(t.shape)}")
    if not bool(((t >= 0) & (t < int(noise_steps))).all()):
        raise ValueError(f"every timestep must lie in [0, {int(noise_steps)})")
    return t


def weighted_mse_loss(pred: torch.Tensor, target: torch.Tensor, t: Optional[torch.Tensor] = None,
                      weights: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, want_grad: bool = True):
    """Per-sample weighted, masked squared error (``wd_weighted_mse_loss``; DESIGN.md "Weighted training loss"):

        loss = mean_b weights[t_b] * sum_i m_bi (pred - target)_bi^2 / sum_i m_bi

    -> (loss [1], d loss / d pred or None, sample_loss [B]): device tensors, ``sample_loss`` the UNWEIGHTED masked mean of every
    sample.  ``pred`` / ``target``: [B, ...] with a multiple of 4 elements per sample; ``weights``: a float tensor [T], finite and
    >= 0, indexed by ``t`` (an integer tensor [B] in [0, T), required with it); ``mask``: the known-region shapes ([h, w],
    [B, 1, h, w] or pred's own) with values in [0, 1] - a sample whose mask is all zero has loss 0 and a zero gradient row.
    Arguments are validated before anything touches the device; the kernel runs on the GPU only."""
    if pred.dim() < 2 or tuple(pred.shape) != tuple(target.shape):
        raise ValueError(f"pred and target must share a shape [B, ...], got {tuple(pred.shape)} and {tuple(target.shape)}")
    B = pred.shape[0]
    n = pred[0].numel() if B else 0
    if B < 1 or n < 4 or n % 4:
        raise ValueError(f"weighted_mse_loss needs B >= 1 and a multiple of 4 elements per sample, got {tuple(pred.shape)}")
    T = 0
    if weights is not None:
        if t is None:
            raise ValueError("weights are indexed by the timesteps: pass t")
        weights = check_loss_weights(weights, torch.as_tensor(weights).numel())
        T = weights.numel()
        t = check_timesteps(t, B, T)
    else:
        t = None  # (nothing reads it)
    if mask is not None:
        if pred.dim() == 4:
            mask = expand_loss_mask(mask, pred.shape)
        else:  # any other [B, ...]: only a mask of pred's own shape has a meaning
            mask = torch.as_tensor(mask)
            if tuple(mask.shape) != tuple(pred.shape):
                raise ValueError(f"loss_mask must have pred's shape {list(pred.shape)}, got {tuple(mask.shape)}")
            mask = expand_loss_mask(mask.reshape(B, 1, 1, n), (B, 1, 1, n))
    if not pred.is_cuda:
        raise N.NativeError("weighted_mse_loss runs on the GPU only (no CPU fallback)")
    lib, dev = N.lib(), pred.device
    pred, target = pred.contiguous().float(), target.contiguous().float()
    if mask is not None:
        mask = mask.to(dev)
    if weights is not None:
        weights, t = weights.to(dev), t.to(dev).long().contiguous()
    grad = torch.empty_like(pred) if want_grad else None
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    sample_loss = torch.empty(B, dtype=torch.float32, device=dev)
    scratch = torch.empty(2 * B, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    N.check(lib.wd_weighted_mse_loss(pred.data_ptr(), target.data_ptr(), mask.data_ptr() if mask is not None else None, B, n,
                                     t.data_ptr() if t is not None else None, weights.data_ptr() if weights is not None else None,
                                     T, grad.data_ptr() if want_grad else None, loss.data_ptr(), sample_loss.data_ptr(), None, 0,
                                     scratch.data_ptr(), st), "wd_weighted_mse_loss")
    return loss, grad, sample_loss


def check_ctc_args(logits, targets, input_lengths, target_lengths):
    """The arguments of ``ctc_loss`` -> (T, B, C, Lmax, targets int64 [B, Lmax], input_lengths int32 [B], target_lengths int32 [B]),
    the three integer tensors on the host.  ``logits``: a float32 tensor [T, B, C] within the kernel's range; ``targets``: integer
    [B, Lmax] (or flat [B * Lmax]) with every id of the first ``target_lengths[b]`` ones in [0, C); ``input_lengths`` in [1, T];
    ``target_lengths`` in [0, Lmax].  Host arithmetic only (on device tensors it costs one small synchronisation each)."""
    D = N.DEFINES
    if not torch.is_tensor(logits) or logits.dim() != 3 or logits.dtype != torch.float32:
        raise ValueError("logits must be a float32 tensor [T, B, C]")
    T, B, C = (int(v) for v in logits.shape)
    if not (1 <= T <= D["WD_CTC_MAX_T"] and B >= 1 and 1 <= C <= D["WD_CTC_MAX_C"]):
        raise ValueError(f"ctc_loss takes 1 <= T <= {D['WD_CTC_MAX_T']}, B >= 1 and 1 <= C <= {D['WD_CTC_MAX_C']}, "
                         f"got logits {list(logits.shape)}")

    def ints(v, name):
        v = torch.as_tensor(v)
        if v.is_floating_point() or v.is_complex() or v.dtype == torch.bool:
            raise ValueError(f"{name} must be an integer tensor, got {v.dtype}")
        return v.detach().cpu().long()

    targets = ints(targets, "targets")
    if targets.dim() == 1 and targets.numel() % B == 0:  # the reference passes the flattened token matrix
        targets = targets.reshape(B, -1)
    if targets.dim() != 2 or targets.shape[0] != B:
        raise ValueError(f"targets must be [B, Lmax] (or flat [B * Lmax]) with B = {B}, got {list(targets.shape)}")
    Lmax = int(targets.shape[1])
    if Lmax > D["WD_CTC_MAX_L"]:
        raise ValueError(f"ctc_loss takes targets of at most {D['WD_CTC_MAX_L']} ids, got {Lmax}")
    il, tl = ints(input_lengths, "input_lengths"), ints(target_lengths, "target_lengths")
    if tuple(il.shape) != (B,) or tuple(tl.shape) != (B,):
        raise ValueError(f"input_lengths and target_lengths must be [{B}], got {list(il.shape)} and {list(tl.shape)}")
    if not bool(((il >= 1) & (il <= T)).all()):
        raise ValueError(f"every input length must lie in [1, {T}]")
    if not bool(((tl >= 0) & (tl <= Lmax)).all()):
        raise ValueError(f"every target length must lie in [0, {Lmax}]")
    used = torch.arange(Lmax)[None, :] < tl[:, None]
    if not bool((((targets >= 0) & (targets < C)) | ~used).all()):
        raise ValueError(f"every target id must lie in [0, {C})")
    return T, B, C, Lmax, targets.contiguous(), il.int().contiguous(), tl.int().contiguous()


def ctc_loss(logits: torch.Tensor, targets, input_lengths, target_lengths, want_grad: bool = True, scale: float = 1.0):
    """``scale * nn.CTCLoss(reduction='sum', zero_infinity=True)(log_softmax(logits, 2), targets, input_lengths, target_lengths)``
    with the blank at class 0 (``trainModifyCondition.py:73,757-799``; the training step passes ``scale = ocr_weight / B``) and
    its gradient with respect to the raw logits, in one ``wd_ctc_loss`` call

    -> (loss [1], dlogits [T, B, C] or None, sample_nll [B]): device tensors; ``sample_nll`` is unscaled, ``inf`` for a sample
    that has no alignment (it adds nothing to the loss and has a zero gradient).  The arguments are validated first
    (``check_ctc_args``); the kernel runs on the GPU only."""
    T, B, C, Lmax, targets, il, tl = check_ctc_args(logits, targets, input_lengths, target_lengths)
    scale = float(scale)
    if not scale == scale or scale in (float("inf"), float("-inf")):
        raise ValueError(f"scale must be finite, got {scale}")
    if not logits.is_cuda:
        raise N.NativeError("ctc_loss runs on the GPU only (no CPU fallback)")
    lib, dev = N.lib(), logits.device
    logits = logits.detach().contiguous()
    targets, il, tl = targets.to(dev), il.to(dev), tl.to(dev)
    grad = torch.empty_like(logits) if want_grad else None
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    sample_nll = torch.empty(B, dtype=torch.float32, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    nbytes = lib.wd_ctc_workspace_bytes(T, B, Lmax)
    work = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    N.check(lib.wd_ctc_loss(logits.data_ptr(), C, T, B, C, targets.data_ptr() if Lmax else None, 1, Lmax, Lmax, il.data_ptr(),
                            tl.data_ptr(), scale, grad.data_ptr() if want_grad else None, C, sample_nll.data_ptr(),
                            loss.data_ptr(), status.data_ptr(), work.data_ptr(), nbytes, st), "wd_ctc_loss")
    return loss, grad, sample_nll


def ctc_greedy_decode(logits, index2letter=None):
    """Best-path decoding of CTC logits [T, B, C] (or [T, C]): the argmax of every step, repeats collapsed, blanks (class 0)
    dropped -> one list of ids per sample, or one string per sample when ``index2letter`` (a mapping or sequence from id to
    letter) is given.  Host code: a device tensor is copied once."""
    logits = torch.as_tensor(logits)
    if logits.dim() == 2:
        logits = logits[:, None, :]
    if logits.dim() != 3 or logits.shape[2] < 1:
        raise ValueError(f"logits must be [T, B, C] or [T, C], got {list(logits.shape)}")
    best = logits.detach().argmax(2).cpu().tolist()  # [T][B]
    out = []
    for b in range(logits.shape[1]):
        seq, prev = [], -1
        for row in best:
            k = row[b]
            if k != prev and k != 0:
                seq.append(k)
            prev = k
        out.append(seq if index2letter is None else "".join(str(index2letter[k]) for k in seq))
    return out


class FusedAdamW:
    """``optim.AdamW(model.parameters(), lr=1e-4)`` (train.py:405) + ``EMA(0.995).step_ema`` (train.py:294,410) in one
    multi-tensor launch.  ``ema_model`` is optional; with it ``step()`` reproduces ``ema.step_ema(ema_model, model)``
    (plain copy for the first ``step_start_ema`` steps, then the moving average).

    ``max_grad_norm`` (a float > 0, or ``inf`` to measure only; default ``None``: off, the launches above and nothing else) is
    ``torch.nn.utils.clip_grad_norm_(params, max_grad_norm)`` folded into the step: ``step()`` first runs the norm pass
    (``wd_grad_sqnorm_multi``: squares summed in double in a fixed order, rounded once to fp32) and then
    ``wd_adamw_multi_scaled``, which multiplies every gradient by ``min(1, max_grad_norm / (norm + 1e-6))`` as it loads it.
    Unlike torch the gradients are NOT scaled in place: ``param.grad`` still holds the unclipped values after ``step()``; the
    coefficient lives in the kernel.  ``grad_norm`` is a device fp32 ``[1]`` tensor with the pre-clip norm of the last step;
    nothing synchronises, the caller reads it when it wants to.  A non-finite norm propagates as in torch (the step is not
    skipped)."""

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, ema_model=None, ema_beta=0.995,
                 step_start_ema=2000, max_grad_norm=None):
        self.params = [p for p in params]
        if not self.params or not self.params[0].is_cuda:
            raise N.NativeError("FusedAdamW needs CUDA parameters (no CPU fallback)")
        if max_grad_norm is not None:
            max_grad_norm = float(max_grad_norm)
            if not max_grad_norm > 0.0:  # (NaN fails the comparison too)
                raise ValueError(f"max_grad_norm must be a positive number or inf, got {max_grad_norm}")
        self.max_grad_norm = max_grad_norm
        # one group in torch.optim's layout: the source of truth for the hyper-parameters (LR schedulers write ``lr`` here)
        self.param_groups = [dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False,
                                  maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                                  params=self.params)]
        self.ema_params = list(ema_model.parameters()) if ema_model is not None else None
        if self.ema_params is not None and len(self.ema_params) != len(self.params):
            raise ValueError("ema_model does not match the parameter list")
        self.ema_beta, self.step_start_ema = ema_beta, step_start_ema
        self.step_count = 0
        self.exp_avg = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
        self.exp_avg_sq = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
        self._table = None
        self._grads = None
        self._grad_ptrs = None
        self._has_state = [False] * len(self.params)  # parameters that have been stepped (torch keeps state only for those)
        # [norm, clip coefficient] of the last step, written by wd_grad_sqnorm_multi and read by wd_adamw_multi_scaled
        # (allocated after the optimiser state, whose placement it therefore leaves alone)
        self._clip_ctl = torch.zeros(2, dtype=torch.float32, device=self.params[0].device)
        self.grad_norm = self._clip_ctl[:1]
        self._partials = None

    lr = property(lambda self: self.param_groups[0]["lr"])
    betas = property(lambda self: self.param_groups[0]["betas"])
    eps = property(lambda self: self.param_groups[0]["eps"])
    weight_decay = property(lambda self: self.param_groups[0]["weight_decay"])

    def zero_grad(self, set_to_none: bool = True):
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    # ---- checkpointing: ``torch.save(optimizer.state_dict(), "models/optim.pt")`` (train.py:316) / resume -------------------
    def state_dict(self):
        """``torch.optim.AdamW.state_dict()`` layout - ``state[i] = {step, exp_avg, exp_avg_sq}`` for every parameter that has
        received a gradient, ``param_groups`` with parameter indices - so the file loads into either optimiser.  The extra
        ``wdiff`` entry (ignored by torch) carries the step counter that also positions the EMA warm-up."""
        state = {}
        if self.step_count > 0:
            for i, p in enumerate(self.params):
                if not self._has_state[i]:
                    continue  # never stepped (no gradient): torch.optim.AdamW holds no state for it either
                state[i] = dict(step=torch.tensor(float(self.step_count)), exp_avg=self.exp_avg[i].clone(),
                                exp_avg_sq=self.exp_avg_sq[i].clone())
        group = {k: v for k, v in self.param_groups[0].items() if k != "params"}
        group["params"] = list(range(len(self.params)))
        return dict(state=state, param_groups=[group],
                    wdiff=dict(step_count=self.step_count, ema_beta=self.ema_beta, step_start_ema=self.step_start_ema))

    def load_state_dict(self, sd):
        groups = sd["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self.params):
            raise ValueError("loaded state dict has a different number of parameter groups / parameters")
        for k, v in groups[0].items():
            if k != "params":
                self.param_groups[0][k] = tuple(v) if k == "betas" else v
        steps = set()
        with torch.no_grad():
            for i, p in enumerate(self.params):
                st = sd["state"].get(i, sd["state"].get(str(i)))
                self._has_state[i] = st is not None
                if st is None:
                    self.exp_avg[i].zero_()
                    self.exp_avg_sq[i].zero_()
                    continue
                if tuple(st["exp_avg"].shape) != tuple(p.shape):
                    raise ValueError(f"optimizer state {i} has shape {tuple(st['exp_avg'].shape)}, parameter {tuple(p.shape)}")
                self.exp_avg[i].copy_(st["exp_avg"])
                self.exp_avg_sq[i].copy_(st["exp_avg_sq"])
                steps.add(int(float(st["step"])))
        if len(steps) > 1:
            raise ValueError(f"per-parameter step counts differ ({sorted(steps)}): one fused launch uses one bias correction")
        extra = sd.get("wdiff", {})
        self.step_count = int(extra.get("step_count", steps.pop() if steps else 0))
        self.ema_beta = extra.get("ema_beta", self.ema_beta)
        self.step_start_ema = extra.get("step_start_ema", self.step_start_ema)

    def _build_table(self):
        lib = N.lib()
        chunk = lib.wd_adamw_chunk()
        recs, c0 = [], 0
        self._grads = []
        for i, p in enumerate(self.params):
            g = p.grad.contiguous() if p.grad is not None else None  # None: torch.optim.AdamW skips the parameter
            self._grads.append(g)
            ema = self.ema_params[i].data_ptr() if self.ema_params is not None else 0
            recs.append(N.WdAdamwTableEntry(p.data_ptr(), g.data_ptr() if g is not None else 0, self.exp_avg[i].data_ptr(),
                                            self.exp_avg_sq[i].data_ptr(), ema, p.numel(), c0))
            c0 += (p.numel() + chunk - 1) // chunk
        raw = torch.frombuffer((N.WdAdamwTableEntry * len(recs))(*recs), dtype=torch.uint8)
        self._table = raw.to(self.params[0].device)
        self._chunks = c0
        if self.max_grad_norm is not None:  # one double per chunk for the norm pass: allocated with the table, not per step
            self._partials = torch.empty(c0, dtype=torch.float64, device=self.params[0].device)
        self._grad_ptrs = [g.data_ptr() if g is not None else 0 for g in self._grads]
        self._has_state = [h or g is not None for h, g in zip(self._has_state, self._grads)]

    def step(self):
        lib = N.lib()
        cur = [p.grad.data_ptr() if p.grad is not None else 0 for p in self.params]
        if self._table is None or cur != self._grad_ptrs:
            self._build_table()
        self.step_count += 1
        if self.ema_params is None:
            mode = 0
        else:
            mode = 1 if (self.step_count - 1) < self.step_start_ema else 2
        st = torch.cuda.current_stream(self.params[0].device).cuda_stream
        hyper = (float(self.lr), float(self.betas[0]), float(self.betas[1]), float(self.eps), float(self.weight_decay),
                 self.step_count, mode, float(self.ema_beta))
        if self.max_grad_norm is None:
            N.check(lib.wd_adamw_multi(self._table.data_ptr(), len(self.params), self._chunks, *hyper, st), "wd_adamw_multi")
        else:
            ctl = self._clip_ctl.data_ptr()
            N.check(lib.wd_grad_sqnorm_multi(self._table.data_ptr(), len(self.params), self._chunks, self._partials.data_ptr(),
                                             self.max_grad_norm, ctl, st), "wd_grad_sqnorm_multi")
            N.check(lib.wd_adamw_multi_scaled(self._table.data_ptr(), len(self.params), self._chunks, *hyper, ctl + 4, st),
                    "wd_adamw_multi_scaled")
        # the kernel changed the parameters (and the EMA copy) behind autograd's back: the engines that packed operands from
        # them must repack before their next use
        from .engine import note_native_write
        note_native_write()


def check_rows(rows, vocab: int) -> tuple:
    """A row list of the row-wise kernels (``wd_row_slots`` / ``wd_adamw_rows``): 1 .. WD_ROWS_MAX distinct integer ids in
    [0, vocab) -> a tuple of ints, in the caller's order.  The C entry points refuse the same lists; this raises first, on the
    host, with a message."""
    try:
        rows = tuple(rows.tolist() if torch.is_tensor(rows) else rows)
    except TypeError:
        raise ValueError(f"rows must be a sequence of writer ids, got {rows!r}") from None
    rmax = N.DEFINES["WD_ROWS_MAX"]
    if not 1 <= len(rows) <= rmax:
        raise ValueError(f"rows must hold 1 .. {rmax} ids, got {len(rows)}")
    if any(isinstance(r, bool) or not isinstance(r, int) for r in rows):
        raise ValueError("rows must be integer ids")
    if any(r < 0 or r >= int(vocab) for r in rows):
        raise ValueError(f"every row must lie in [0, {int(vocab)})")
    if len(set(rows)) != len(rows):
        raise ValueError("rows must be distinct")
    return rows


class RowAdamW:
    """AdamW (+ EMA) over a few rows of one embedding table, every other parameter frozen: the optimiser of embedding-only
    fitting (DESIGN.md "Fitting new writers").  ``table_param`` is ``model.label_emb.weight``, ``rows`` the ids being fitted.  It
    holds compact ``[R, c]`` buffers - ``row_grad`` (written by the frozen backward plan of ``TrainStep``), ``exp_avg``,
    ``exp_avg_sq`` - and ``step()`` is one ``wd_adamw_rows`` launch, after the norm pass of ``wd_grad_sqnorm_multi`` over
    ``row_grad`` when ``max_grad_norm`` is given (``grad_norm`` then holds the pre-clip norm, as in ``FusedAdamW``).

    ``anchor``: None - plain decoupled decay towards zero, ``wd_adamw_multi``'s arithmetic; "init" - the rows' values at
    construction; a float tensor [R, c].  With an anchor the decay pulls towards it, p -= lr * weight_decay * (p - a): decay
    towards zero would drag a fitted row towards the writer-free point.  ``ema_model``: a model with a table of the same shape
    (grown by the same ``add_writers`` call); its rows follow ``step_start_ema`` as in ``FusedAdamW``, nothing else of it is
    touched."""

    def __init__(self, table_param, rows, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, anchor=None, ema_model=None,
                 ema_beta=0.995, step_start_ema=2000, max_grad_norm=None):
        import ctypes as C
        if not torch.is_tensor(table_param) or table_param.dim() != 2 or table_param.dtype != torch.float32:
            raise ValueError("table_param must be a 2-d fp32 embedding table")
        vocab, c = table_param.shape
        self.rows = check_rows(rows, vocab)
        if c % 4:
            raise ValueError(f"the table's width must be a multiple of 4, got {c}")
        if not table_param.is_cuda:
            raise N.NativeError("RowAdamW needs a CUDA table (no CPU fallback)")
        if not table_param.is_contiguous():
            raise ValueError("table_param must be contiguous")
        if max_grad_norm is not None:
            max_grad_norm = float(max_grad_norm)
            if not max_grad_norm > 0.0:
                raise ValueError(f"max_grad_norm must be a positive number or inf, got {max_grad_norm}")
        self.max_grad_norm = max_grad_norm
        self.table = table_param
        self.params = [table_param]
        self.param_groups = [dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, params=self.params)]
        self.ema_beta, self.step_start_ema = ema_beta, step_start_ema
        self.ema_table = None
        if ema_model is not None:
            et = getattr(getattr(ema_model, "label_emb", None), "weight", None)
            if et is None or tuple(et.shape) != (vocab, c) or et.device != table_param.device or not et.is_contiguous():
                raise ValueError("ema_model does not hold a writer table of the same shape on the same device")
            self.ema_table = et
        dev, R = table_param.device, len(self.rows)
        self._rows_c = (C.c_int * R)(*self.rows)
        self.step_count = 0
        self.row_grad = torch.zeros(R, c, dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros(R, c, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(R, c, dtype=torch.float32, device=dev)
        if anchor is None:
            self.anchor = None
        elif isinstance(anchor, str):
            if anchor != "init":
                raise ValueError(f"anchor must be None, 'init' or a float tensor [{R}, {c}], not {anchor!r}")
            self.anchor = table_param.detach()[list(self.rows)].clone()
        else:
            anchor = torch.as_tensor(anchor)
            if not anchor.is_floating_point() or tuple(anchor.shape) != (R, c):
                raise ValueError(f"anchor must be None, 'init' or a float tensor [{R}, {c}], got {tuple(anchor.shape)}")
            self.anchor = anchor.detach().to(device=dev, dtype=torch.float32).contiguous().clone()
        self._clip_ctl = torch.zeros(2, dtype=torch.float32, device=dev)
        self.grad_norm = self._clip_ctl[:1]
        self._norm_table = self._partials = None

    lr = property(lambda self: self.param_groups[0]["lr"])
    betas = property(lambda self: self.param_groups[0]["betas"])
    eps = property(lambda self: self.param_groups[0]["eps"])
    weight_decay = property(lambda self: self.param_groups[0]["weight_decay"])

    def zero_grad(self, set_to_none: bool = True):
        self.row_grad.zero_()

    def bind_grad(self, buf: torch.Tensor):
        """Makes ``buf`` (fp32 [R, c] on the table's device: a frozen-trunk plan's ``row_grad``) the gradient ``step()`` reads."""
        if buf.dtype != torch.float32 or tuple(buf.shape) != tuple(self.exp_avg.shape) or buf.device != self.table.device or \
                not buf.is_contiguous():
            raise ValueError(f"row_grad must be a contiguous fp32 {list(self.exp_avg.shape)} tensor on the table's device")
        self.row_grad = buf
        self._norm_table = None  # (it holds the old buffer's address)

    def state_dict(self):
        """The rows, the step and the three buffers (plus the anchor and the hyper-parameters)."""
        group = {k: v for k, v in self.param_groups[0].items() if k != "params"}
        return dict(rows=list(self.rows), step_count=self.step_count, row_grad=self.row_grad.clone(), exp_avg=self.exp_avg.clone(),
                    exp_avg_sq=self.exp_avg_sq.clone(), anchor=None if self.anchor is None else self.anchor.clone(),
                    param_group=group, ema_beta=self.ema_beta, step_start_ema=self.step_start_ema)

    def load_state_dict(self, sd):
        if tuple(sd["rows"]) != self.rows:
            raise ValueError(f"loaded state is for rows {list(sd['rows'])}, this optimiser fits {list(self.rows)}")
        for name in ("row_grad", "exp_avg", "exp_avg_sq"):
            if tuple(sd[name].shape) != tuple(self.row_grad.shape):
                raise ValueError(f"{name} has shape {tuple(sd[name].shape)}, expected {tuple(self.row_grad.shape)}")
        if (sd.get("anchor") is None) != (self.anchor is None):
            raise ValueError("loaded state and this optimiser disagree on having an anchor")
        with torch.no_grad():
            for name in ("row_grad", "exp_avg", "exp_avg_sq"):
                getattr(self, name).copy_(sd[name])
            if self.anchor is not None:
                self.anchor.copy_(sd["anchor"])
        for k, v in sd.get("param_group", {}).items():
            self.param_groups[0][k] = tuple(v) if k == "betas" else v
        self.step_count = int(sd["step_count"])
        self.ema_beta = sd.get("ema_beta", self.ema_beta)
        self.step_start_ema = sd.get("step_start_ema", self.step_start_ema)

    def step(self):
        lib, dev = N.lib(), self.table.device
        vocab, c = self.table.shape
        self.step_count += 1
        mode = 0 if self.ema_table is None else (1 if (self.step_count - 1) < self.step_start_ema else 2)
        st = torch.cuda.current_stream(dev).cuda_stream
        gscale = None
        if self.max_grad_norm is not None:
            if self._norm_table is None:  # a one-entry wd_adamw_multi table over row_grad: the norm pass reads g and n only
                chunk = lib.wd_adamw_chunk()
                n = self.row_grad.numel()
                rec = N.WdAdamwTableEntry(0, self.row_grad.data_ptr(), 0, 0, 0, n, 0)
                self._norm_table = torch.frombuffer((N.WdAdamwTableEntry * 1)(rec), dtype=torch.uint8).to(dev)
                self._chunks = (n + chunk - 1) // chunk
                self._partials = torch.empty(self._chunks, dtype=torch.float64, device=dev)
            N.check(lib.wd_grad_sqnorm_multi(self._norm_table.data_ptr(), 1, self._chunks, self._partials.data_ptr(),
                                             self.max_grad_norm, self._clip_ctl.data_ptr(), st), "wd_grad_sqnorm_multi")
            gscale = self._clip_ctl.data_ptr() + 4
        N.check(lib.wd_adamw_rows(self.table.data_ptr(), c, c, self._rows_c, len(self.rows), vocab, self.row_grad.data_ptr(),
                                  self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                                  None if self.anchor is None else self.anchor.data_ptr(),
                                  None if self.ema_table is None else self.ema_table.data_ptr(), c, float(self.lr),
                                  float(self.betas[0]), float(self.betas[1]), float(self.eps), float(self.weight_decay),
                                  self.step_count, mode, float(self.ema_beta), gscale, st), "wd_adamw_rows")
        # the kernel changed the table (and the EMA copy) behind autograd's back: every engine repacks before its next use
        from .engine import note_native_write
        note_native_write()
