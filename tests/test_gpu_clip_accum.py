"""Gradient accumulation (``TrainStep(accumulate=A)``) and global-norm clipping (``FusedAdamW(max_grad_norm=...)``) on the GPU:

  1. the kernels at the optimiser level - ``wd_grad_sqnorm_multi`` against tests/_clip_ref.py (2^-23 relative: one rounding of
     a sum that is exact in double; bit-identical on a second run; an unaligned gradient view), ``wd_adamw_multi_scaled`` in
     the clipped regime against torch-CPU AdamW on the pre-scaled gradients and in the unclipped regime bit-equal to the plain
     kernel, ``wd_grad_accumulate`` exact against np.float32 arithmetic;
  2. ``TrainStep`` on the SMALL config with micro-batches of 4: the accumulated gradient against the float64 oracle on the whole
     batch (plain, with dropout, two data-parallel ranks), the calls inside a group inert, graph = eager, the eps / mask keying,
     clipping through the step, and the default settings' launches."""
import collections
import copy
import functools
import os
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ddpm_oracle as D  # noqa: E402
from oracle import unet_oracle as U  # noqa: E402
from tests import _clip_ref as R  # noqa: E402
from tests._common import SMALL, join_all, make_args  # noqa: E402
from tests.test_gpu_dropout import dropped_resblock  # noqa: E402  (U.resblock with the host mask of tests/_dropout_ref.py)
from tests.test_gpu_training import _close  # noqa: E402
from worddiffusion_amd import Diffusion, UNetModel  # noqa: E402
from worddiffusion_amd import _native as N  # noqa: E402
from worddiffusion_amd.optim import FusedAdamW  # noqa: E402
from worddiffusion_amd.synthetic import fill_module_, synthetic_inputs, synthetic_tensor  # noqa: E402
from worddiffusion_amd.training import TrainStep  # noqa: E402

DEV = "cuda:0"
CHUNK = 8192
SIZES = [1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5, CHUNK + 1, 7]  # test_fused_adamw_at_chunk_edges
NONE_AT = 5                                                             # this parameter never gets a gradient
SPREAD = [1e-4, 1e-2, 1.0, 10.0, 1e2, None, 1e3]                        # per-tensor gradient magnitudes


# ------------------------------------------------------------------------------------------ 1. optimiser level
def _tensors(seed, scales=None, unaligned_at=None):
    """(initial values, device parameters with .grad buffers, CPU gradients).  unaligned_at: that gradient is a view one
    element into a larger buffer (4 bytes past a 16-byte boundary)."""
    g = torch.Generator().manual_seed(seed)
    init = [torch.randn(n, generator=g) for n in SIZES]
    params = [torch.nn.Parameter(v.clone().to(DEV)) for v in init]
    grads = []
    for i, (p, n) in enumerate(zip(params, SIZES)):
        if i == NONE_AT:
            grads.append(None)
            continue
        gr = torch.randn(n, generator=g) * (1.0 if scales is None else scales[i])
        grads.append(gr)
        if i == unaligned_at:
            buf = torch.zeros(n + 1, device=DEV)
            p.grad = buf[1:]
            assert p.grad.data_ptr() % 16 == 4
            p.grad.copy_(gr.to(DEV))
        else:
            p.grad = gr.to(DEV)
    return init, params, grads


@pytest.mark.parametrize("unaligned_at", [None, 4, 1])
def test_grad_norm_against_the_reference(unaligned_at):
    """Magnitudes from 1e-4 to 1e3 per tensor: an fp32 accumulation would lose the small tensors' digits."""
    _, params, grads = _tensors(1, SPREAD, unaligned_at)
    opt = FusedAdamW(params, lr=1e-3, max_grad_norm=float("inf"))
    assert opt.grad_norm.shape == (1,) and opt.grad_norm.dtype == torch.float32 and opt.grad_norm.is_cuda
    opt.step()
    torch.cuda.synchronize()
    first = opt.grad_norm.cpu().clone()
    want = R.global_norm(grads)
    rel = abs(float(first) - float(want)) / float(want)
    print(f"norm {float(first):.9g} reference {float(want):.9g} relative difference {rel:.2e}")
    assert rel <= 2.0 ** -23
    assert float(opt._clip_ctl[1].cpu()) == 1.0
    opt.step()  # the same gradients again (the parameters moved, the norm must not)
    torch.cuda.synchronize()
    assert torch.equal(opt.grad_norm.cpu(), first)
    for p, g in zip(params, grads):  # the gradients are not modified in place
        assert g is None or torch.equal(p.grad.cpu(), g)


class _Holder(torch.nn.Module):
    def __init__(self, ps):
        super().__init__()
        self.ps = torch.nn.ParameterList(ps)


def test_clipped_adamw_against_torch_on_prescaled_gradients():
    """max_grad_norm about half the norm of the first step's gradients (the later ones are larger).  Reference: the CPU
    gradients multiplied in fp32 by the _clip_ref coefficient, torch.optim.AdamW(foreach=False), EMA as EMA.step_ema."""
    g = torch.Generator().manual_seed(2)
    init = [torch.randn(n, generator=g) for n in SIZES]
    params = [torch.nn.Parameter(v.clone().to(DEV)) for v in init]
    cpu = [torch.nn.Parameter(v.clone()) for v in init]
    ema_init = [torch.randn(n, generator=g) for n in SIZES]
    ema = [torch.nn.Parameter(v.clone().to(DEV), requires_grad=False) for v in ema_init]
    ema_ref = [v.clone() for v in ema_init]
    lr, beta = 1e-3, 0.995
    step_grads = [[None if i == NONE_AT else torch.randn(n, generator=g) * (0.1 * s) for i, n in enumerate(SIZES)]
                  for s in range(1, 8)]
    max_norm = 0.5 * float(R.global_norm(step_grads[0]))
    opt = FusedAdamW(params, lr=lr, ema_model=_Holder(ema), ema_beta=beta, step_start_ema=0, max_grad_norm=max_norm)
    ref = torch.optim.AdamW(cpu, lr=lr, foreach=False)
    for i, p in enumerate(params):
        if i != NONE_AT:
            p.grad = torch.zeros_like(p)
    for s, grads in enumerate(step_grads, start=1):
        norm, coef, scaled = R.clipped(grads, max_norm)
        assert coef < 0.51
        for p, c, gr, sc in zip(params, cpu, grads, scaled):
            if gr is not None:
                c.grad = torch.from_numpy(sc).clone()
                p.grad.copy_(gr.to(DEV))
        opt.step()
        ref.step()
        with torch.no_grad():
            for e, c in zip(ema_ref, cpu):
                e.copy_(e * beta + (1 - beta) * c.detach())
        torch.cuda.synchronize()
        assert abs(float(opt.grad_norm.cpu()) - float(norm)) <= 2.0 ** -23 * float(norm)
        if s not in (1, 7):
            continue
        for i, (p, c) in enumerate(zip(params, cpu)):
            if i == NONE_AT:
                assert torch.equal(p.detach().cpu(), init[i])
                assert not bool(opt.exp_avg[i].any()) and not bool(opt.exp_avg_sq[i].any())
            else:
                st = ref.state[c]
                for what, got, want in (("p", p, c), ("m", opt.exp_avg[i], st["exp_avg"]), ("v", opt.exp_avg_sq[i], st["exp_avg_sq"])):
                    ok, rel, _ = _close(got, want)
                    assert ok, (what, SIZES[i], s, rel)
            ok, rel, _ = _close(ema[i], ema_ref[i])
            assert ok, ("ema", SIZES[i], s, rel)


@pytest.mark.parametrize("factor", [10.0, float("inf")])
def test_unclipped_adamw_is_the_plain_kernel_bit_for_bit(factor):
    def run(max_grad_norm):
        init, params, grads = _tensors(3, SPREAD)
        ema = [torch.nn.Parameter(torch.full_like(p, 0.25), requires_grad=False) for p in params]
        opt = FusedAdamW(params, lr=1e-3, ema_model=_Holder(ema), step_start_ema=0, max_grad_norm=max_grad_norm)
        for _ in range(3):
            opt.step()
        torch.cuda.synchronize()
        return params, opt.exp_avg, opt.exp_avg_sq, ema, grads

    plain = run(None)
    got = run(factor * float(R.global_norm(plain[4])))
    for a, b in zip(plain[:4], got[:4]):
        for x, y in zip(a, b):
            assert torch.equal(x.detach(), y.detach())


@pytest.mark.parametrize("scale", [0.5, 1.0 / 3.0])
@pytest.mark.parametrize("n", [1, 63, 8193])
@pytest.mark.parametrize("off_dst,off_src", [(0, 0), (1, 1), (0, 1)], ids=["aligned", "offset1", "misaligned"])
def test_grad_accumulate_exact(n, scale, off_dst, off_src):
    """dst = scale * (overwrite ? src : dst + src), every operation one fp32 rounding; with overwrite a NaN-filled dst is never
    read.  The guard elements around dst stay NaN (nothing is written out of range)."""
    lib = N.lib()
    rs = np.random.RandomState(n)
    src = rs.standard_normal(n).astype(np.float32)
    old = rs.standard_normal(n).astype(np.float32)
    sc = np.float32(scale)
    st = torch.cuda.current_stream().cuda_stream
    for overwrite in (1, 0):
        dbuf = torch.full((n + 8,), float("nan"), device=DEV)
        sbuf = torch.zeros(n + 8, device=DEV)
        d, s = dbuf[4 + off_dst: 4 + off_dst + n], sbuf[4 + off_src: 4 + off_src + n]
        s.copy_(torch.from_numpy(src))
        if not overwrite:
            d.copy_(torch.from_numpy(old))
        N.check(lib.wd_grad_accumulate(d.data_ptr(), s.data_ptr(), n, overwrite, scale, st), "wd_grad_accumulate")
        torch.cuda.synchronize()
        want = sc * (src if overwrite else old + src)
        assert want.dtype == np.float32
        assert np.array_equal(d.cpu().numpy(), want)
        out = dbuf.cpu()
        assert bool(torch.isnan(out[: 4 + off_dst]).all()) and bool(torch.isnan(out[4 + off_dst + n:]).all())
        assert np.array_equal(s.cpu().numpy(), src)


def test_validation():
    with pytest.raises(ValueError):
        TrainStep(None, None, None, accumulate=0)
    p = [torch.nn.Parameter(torch.zeros(4, device=DEV))]
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            FusedAdamW(p, max_grad_norm=bad)
    sd = FusedAdamW(p, max_grad_norm=1.0).state_dict()
    assert sd.keys() == FusedAdamW(p).state_dict().keys() and sd["param_groups"] == FusedAdamW(p).state_dict()["param_groups"]


# ------------------------------------------------------------------------------------------ 2. TrainStep
HW = (4, 8)
P_DROP, DROP_SEED = 0.1, 77


def _batch(B):
    inp = synthetic_inputs(B, seed=9, hw=HW, num_classes=SMALL["num_classes"])
    eps = torch.randn(inp["x"].shape, generator=torch.Generator().manual_seed(4))
    return inp, eps


def _setup(lr=0.0, ema=False, dropout=0.0, model_seed=31, **optkw):
    m = UNetModel(args=make_args(device=DEV), **SMALL, dropout=dropout)
    fill_module_(m, model_seed)
    m = m.to(DEV).train()
    ema_m = copy.deepcopy(m).eval().requires_grad_(False) if ema else None
    opt = FusedAdamW(m.parameters(), lr=lr, ema_model=ema_m, step_start_ema=0, **optkw)
    diff = Diffusion(noise_steps=1000, img_size=(32, 64), args=make_args(device=DEV))
    return m, ema_m, opt, diff


@functools.lru_cache(maxsize=4)
def oracle64(B, dropout=False, model_seed=31):
    """float64 oracle on all B samples (x_t = noise_images(x0, t, eps)) -> MSE -> autograd: (loss, {name: grad}, global norm).
    dropout: the ResBlocks carry the host mask at rows 0 .. B-1."""
    inp, eps = _batch(B)
    x = D.noise_images(D.schedule(1000)[2], inp["x"], inp["t"], eps)
    sd = {k: torch.from_numpy(synthetic_tensor(k, s, model_seed)).double().requires_grad_(True)
          for k, s in U.state_dict_shapes(SMALL, "base")}
    orc = U.UNetOracle(SMALL, sd, "base", False)
    with pytest.MonkeyPatch.context() as mp:
        if dropout:
            keys = [k for k, _ in U.state_dict_shapes(SMALL, "base") if k.endswith("out_layers.3.weight")]
            layers = {k[: -len("out_layers.3.weight")]: i for i, k in enumerate(keys)}
            mp.setattr(U, "resblock", dropped_resblock(layers, DROP_SEED, 0, P_DROP))
        pred = orc(x.double(), inp["t"], inp["context"], inp["y"], None)
    loss = torch.nn.functional.mse_loss(pred, eps.double())
    loss.backward()
    grads = {k: v.grad for k, v in sd.items() if v.grad is not None}
    norm = float(torch.sqrt(sum((g ** 2).sum() for g in grads.values())))
    return float(loss.detach()), grads, norm


def _check_grads(grads, gref, label):
    """The project's gradient bound, per parameter: ||g - ref|| < 2e-4 ||ref|| + 1e-7, over the same set of parameters."""
    assert set(grads) == set(gref), sorted(set(grads) ^ set(gref))[:10]
    worst, bad = ("", 0.0), []
    for k, r in gref.items():
        g = grads[k].detach().cpu().double()
        assert tuple(g.shape) == tuple(r.shape), k
        err, rn = float((g - r).norm()), float(r.norm())
        if rn > 1e-6 and err / rn > worst[1]:
            worst = (k, err / rn)
        if not err < 2e-4 * rn + 1e-7:
            bad.append((k, err, rn))
    print(f"{label}: worst relative gradient error {worst[1]:.2e} ({worst[0]})")
    assert not bad, f"{len(bad)} gradients off the reference: {bad[:8]}"


def _call(step, inp, eps, lo, hi, noise=True):
    sl = slice(lo, hi)
    return step(inp["x"][sl].to(DEV), inp["context"][sl].to(DEV), inp["y"][sl].to(DEV), t=inp["t"][sl],
                noise=eps[sl].to(DEV) if noise else None)


def _two_calls(step, inp, eps):
    losses = [float(_call(step, inp, eps, 4 * a, 4 * a + 4).cpu()) for a in range(2)]
    torch.cuda.synchronize()
    return losses


@pytest.mark.parametrize("dropout", [False, True], ids=["plain", "dropout"])
def test_accumulated_gradient_against_the_oracle(dropout):
    """accumulate=2 over the two halves of an 8-sample batch, lr = 0: the arena after the second call is the mean of the two
    half-batch gradients = the gradient of the MSE over all 8.  dropout: the masks of call c sit at rows 4c .. 4c+3, the rows one
    B = 8 call would use."""
    m, _, opt, diff = _setup(dropout=P_DROP if dropout else 0.0)
    step = TrainStep(m, diff, opt, seed=DROP_SEED, accumulate=2)
    inp, eps = _batch(8)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    losses = _two_calls(step, inp, eps)
    loss_ref, gref, _ = oracle64(8, dropout)
    assert (step.micro_index, step.optimizer_steps, step.step_index, opt.step_count) == (0, 1, 2, 1)
    assert step._acc is not None and step._acc.numel() == step.eng.grad_arena().numel()
    _check_grads({k: g.clone() for k, g in step.eng.grads().items()}, gref, f"accumulate=2 x B=4, dropout={dropout}")
    mean = 0.5 * (losses[0] + losses[1])
    print(f"losses {losses}, mean {mean:.9g}, oracle {loss_ref:.9g}")
    assert abs(mean - loss_ref) <= 1e-5 * abs(loss_ref)
    for k, p in m.named_parameters():  # param.grad are the arena views the optimiser stepped on
        assert p.grad is None or p.grad.data_ptr() == step.eng.grads()[k].data_ptr()
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), f"{k}: lr = 0 moved the parameter"


def test_first_call_of_a_group_is_inert():
    m, ema_m, opt, diff = _setup(lr=1e-4, ema=True)
    with torch.no_grad():
        for p in ema_m.parameters():
            p.mul_(0.5)  # (an EMA that differs from the weights: a step would show)
    step = TrainStep(m, diff, opt, accumulate=2)
    inp, eps = _batch(8)
    p0 = [p.detach().clone() for p in m.parameters()]
    e0 = [p.detach().clone() for p in ema_m.parameters()]
    loss = _call(step, inp, eps, 0, 4)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss.cpu()))
    assert (opt.step_count, step.micro_index, step.optimizer_steps, step.step_index) == (0, 1, 0, 1)
    for p, a, e, b, m1, v1 in zip(m.parameters(), p0, ema_m.parameters(), e0, opt.exp_avg, opt.exp_avg_sq):
        assert torch.equal(p.detach(), a) and torch.equal(e.detach(), b)
        assert not bool(m1.any()) and not bool(v1.any())
        assert p.grad is None
    assert torch.equal(step._acc, step.eng.grad_arena()) and bool(step._acc.any())
    _call(step, inp, eps, 4, 8)
    torch.cuda.synchronize()
    assert (opt.step_count, step.micro_index, step.optimizer_steps) == (1, 0, 1)
    assert any(not torch.equal(p.detach(), a) for p, a in zip(m.parameters(), p0))
    assert any(not torch.equal(e.detach(), b) for e, b in zip(ema_m.parameters(), e0))


def test_graph_equals_eager_and_bucketed():
    """The same two calls through the captured graph, eagerly, and through the three-segment form (prefix folds): arena and
    parameters bit-equal."""
    inp, eps = _batch(8)
    runs = []
    for kw in (dict(use_graph=True), dict(use_graph=False), dict(use_graph=True, bucketed=True)):
        m, _, opt, diff = _setup(lr=1e-4)
        step = TrainStep(m, diff, opt, accumulate=2, **kw)
        _two_calls(step, inp, eps)
        assert len(step.segments) == (3 if kw.get("bucketed") else 0)
        runs.append((step.eng.grad_arena().clone(), [p.detach().clone() for p in m.parameters()], step))
    assert runs[0][2]._graph is not None and runs[1][2]._graph is None
    for arena, params, _ in runs[1:]:
        assert torch.equal(arena, runs[0][0])
        for a, b in zip(params, runs[0][1]):
            assert torch.equal(a, b)
    assert bool(runs[0][0].any())


def test_keying_two_calls_of_4_draw_what_one_call_of_8_draws():
    """noise=None: the eps rows of call c are keyed by the global row (c * world + rank) * B + b and step_index counts calls, so
    calls 2k and 2k + 1 of an accumulate=2 run draw the halves of call k of a B = 8 run (optimiser steps 0 and 1)."""
    inp, eps = _batch(8)
    m, _, opt, diff = _setup()
    big = TrainStep(m, diff, opt, seed=123)
    whole = []
    for _ in range(2):
        _call(big, inp, eps, 0, 8, noise=False)
        torch.cuda.synchronize()
        whole.append(big._eps.clone())
    m2, _, opt2, diff2 = _setup()
    acc = TrainStep(m2, diff2, opt2, seed=123, accumulate=2)
    for k in range(2):
        for a in range(2):
            _call(acc, inp, eps, 4 * a, 4 * a + 4, noise=False)
            torch.cuda.synchronize()
            assert torch.equal(acc._eps, whole[k][4 * a: 4 * a + 4]), (k, a)
    assert acc.step_index == 4 and acc.optimizer_steps == 2 and big.step_index == 2
    assert not torch.equal(whole[0], whole[1])


def test_clipping_through_train_step():
    loss_ref, gref, norm_ref = oracle64(8)
    inp, eps = _batch(8)
    # lr = 0: the measured norm is the norm of the mean gradient
    m, _, opt, diff = _setup(max_grad_norm=0.5 * norm_ref)
    step = TrainStep(m, diff, opt, accumulate=2)
    _two_calls(step, inp, eps)
    assert step.last_grad_norm is opt.grad_norm
    got = float(step.last_grad_norm.cpu())
    print(f"last_grad_norm {got:.9g}, float64 oracle {norm_ref:.9g}")
    assert abs(got - norm_ref) <= 2e-4 * norm_ref
    # lr = 1e-4: the parameters after the step = a torch-CPU AdamW step on the HIP gradients scaled by the reference coefficient
    m, _, opt, diff = _setup(lr=1e-4, max_grad_norm=0.5 * norm_ref)
    step = TrainStep(m, diff, opt, accumulate=2)
    cpu = {k: torch.nn.Parameter(p.detach().cpu().clone()) for k, p in m.named_parameters()}
    _two_calls(step, inp, eps)
    names = [k for k, p in m.named_parameters() if p.grad is not None]
    hip = [m.get_parameter(k).grad.detach().cpu().contiguous() for k in names]
    norm, coef, scaled = R.clipped(hip, 0.5 * norm_ref)
    assert 0.49 < float(coef) < 0.51 and float(step.last_grad_norm.cpu()) == pytest.approx(float(norm), rel=2.0 ** -22)
    for k, s in zip(names, scaled):
        cpu[k].grad = torch.from_numpy(np.ascontiguousarray(s)).reshape(cpu[k].shape)
    torch.optim.AdamW(list(cpu.values()), lr=1e-4, foreach=False).step()
    moved = 0
    for k, p in m.named_parameters():
        ok, rel, _ = _close(p, cpu[k])
        assert ok, (k, rel)
        moved += int(k in names)
    assert moved == len(names) > 100


def test_default_settings_launch_what_the_parent_launches(monkeypatch):
    """accumulate=1, max_grad_norm=None: the plan is the one an accumulating step builds (accumulation never touches the launch
    lists) and the optimiser side is the single wd_adamw_multi launch - none of the new entry points runs."""
    lib = N.lib()
    calls = collections.Counter()
    for name in ("wd_adamw_multi", "wd_adamw_multi_scaled", "wd_grad_sqnorm_multi", "wd_grad_accumulate", "wd_graph_launch"):
        def spy(*a, _f=getattr(lib, name), _n=name):
            calls[_n] += 1
            return _f(*a)
        monkeypatch.setattr(lib, name, spy)
    inp, eps = _batch(8)
    m, _, opt, diff = _setup(lr=1e-4)
    step = TrainStep(m, diff, opt)
    assert step.accumulate == 1 and opt.max_grad_norm is None
    for _ in range(2):
        _call(step, inp, eps, 0, 4)
    torch.cuda.synchronize()
    assert dict(calls) == {"wd_adamw_multi": 2, "wd_graph_launch": 2}
    assert step._acc is None and opt._partials is None and (step.micro_index, step.optimizer_steps) == (0, 2)
    names = lambda P: ([fn.__name__ for fn, _, _ in P.step], [fn.__name__ for fn, _, _ in P.bwd])  # noqa: E731
    calls.clear()
    m2, _, opt2, diff2 = _setup(lr=1e-4, max_grad_norm=1.0)
    step2 = TrainStep(m2, diff2, opt2, accumulate=2)
    for a in range(2):
        _call(step2, inp, eps, 4 * a, 4 * a + 4)
    torch.cuda.synchronize()
    assert names(step2._P) == names(step._P)
    assert dict(calls) == {"wd_adamw_multi_scaled": 1, "wd_grad_sqnorm_multi": 1, "wd_grad_accumulate": 2, "wd_graph_launch": 2}


# ------------------------------------------------------------------------------------------ two ranks on one GPU
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_main(rank, world, port, out_path):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        m, _, opt, diff = _setup()
        step = TrainStep(m, diff, opt, accumulate=2)
        assert step.world == world
        inp, eps = _batch(16)
        for a in range(2):
            lo = (2 * a + rank) * 4
            _call(step, inp, eps, lo, lo + 4)
        torch.cuda.synchronize()
        if rank == 0:
            torch.save({"grads": {k: g.detach().cpu() for k, g in step.eng.grads().items()}, "segments": len(step.segments),
                        "counts": (step.micro_index, step.optimizer_steps, opt.step_count)}, out_path)
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_two_ranks_accumulate_to_the_16_sample_gradient(tmp_path):
    """world 2 x accumulate 2 x B = 4 through the bucketed path (gloo, both ranks on this GPU): rank r, call a trains on samples
    [(2a + r) * 4, +4) of a 16-sample batch; collectives on the second call only, final scale 1 / 4."""
    import torch.multiprocessing as mp
    out = str(tmp_path / "rank0.pt")
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    join_all(procs, 600)
    got = torch.load(out, weights_only=True)
    assert got["segments"] == 3 and tuple(got["counts"]) == (0, 1, 1)
    _check_grads(got["grads"], oracle64(16)[1], "2 ranks x accumulate=2 x B=4")
