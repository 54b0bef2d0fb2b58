"""Fitting new writers end to end: ``TrainStep`` over a ``RowAdamW``, ``fit_writers`` and ``score_writers``.  SMALL base model
(c = ted = 256, 4 x 8 latents), two rows added, B = 4 with y = [new0, old, new1, new0].

The optimiser's arithmetic is pinned bit for bit in test_gpu_rowopt.py and the frozen plan's gradient in
test_gpu_writer_fit_plan.py, so the trajectory is checked step by step: before every call the rows are read back, float64 autograd
of the oracle gives the gradient AT those values, and ``opt.row_grad`` after the call is held to the project's gradient bar
(||g - ref|| < 2e-4 ||ref|| + 1e-7).  No trajectory tolerance is invented."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ddpm_oracle as D  # noqa: E402
from oracle import unet_oracle as U  # noqa: E402
from tests._common import SMALL, make_args, max_rel  # noqa: E402
from tests._train_ref import DEV, case_inputs, train_model  # noqa: E402
from worddiffusion_amd import Diffusion, fit_writers, score_writers  # noqa: E402
from worddiffusion_amd.optim import FusedAdamW, RowAdamW  # noqa: E402
from worddiffusion_amd.training import TrainStep  # noqa: E402

SEEDS = (41, 9, 6)
B, HW, T = 4, (4, 8), 1000
TS = torch.tensor([30, 400, 700, 990])
OLD = SMALL["num_classes"]
ROWS = (OLD, OLD + 1)
INIT = [4, 7]


def diffusion():
    return Diffusion(noise_steps=T, img_size=(32, 64), args=make_args(device=DEV))


def grown_model(with_ema=False):
    m = train_model(SMALL, "base", False, SEEDS[0])
    ema = copy.deepcopy(m).eval().requires_grad_(False) if with_ema else None
    assert m.add_writers(2, init=INIT) == list(ROWS)
    if ema is not None:
        assert ema.add_writers(2, init=INIT) == list(ROWS)  # (the caller grows the EMA copy with the same call)
    return (m, ema) if with_ema else m


def inputs():
    x0, inp, eps = case_inputs(SMALL, B, HW, 0, SEEDS)
    inp["y"] = torch.tensor([ROWS[0], 3, ROWS[1], ROWS[0]])
    return x0, inp, eps


def call(step, **kw):
    x0, inp, eps = inputs()
    loss = step(x0.to(DEV), inp["context"].to(DEV), inp["y"].to(DEV), t=TS, noise=eps.to(DEV), **kw).clone()
    torch.cuda.synchronize()
    return loss


def oracle(m):
    sd = {k: v.detach().cpu().double().requires_grad_(k == "label_emb.weight") for k, v in m.state_dict().items()}
    return U.UNetOracle(dict(SMALL, num_classes=m.num_classes), sd, "base", False), sd


def gradient64(m):
    """float64 autograd of the oracle at the model's present weights: d MSE(noised batch) / d label_emb.weight at ROWS."""
    x0, inp, eps = inputs()
    orc, sd = oracle(m)
    x_t = D.noise_images(D.schedule(T)[2], x0, TS, eps)
    pred = orc(x_t.double(), TS, inp["context"], inp["y"], None)
    torch.nn.functional.mse_loss(pred, eps.double()).backward()
    return sd["label_emb.weight"].grad[list(ROWS)]


def snapshot(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def assert_only_rows_moved(m, before, what):
    for k, v in m.state_dict().items():
        if k == "label_emb.weight":
            others = [r for r in range(v.shape[0]) if r not in ROWS]
            assert torch.equal(v[others].view(torch.int32), before[k][others].view(torch.int32)), f"{what}: an unfitted row moved"
        else:
            assert torch.equal(v, before[k]), f"{what}: {k} moved"


# ------------------------------------------------------------------------------------------------------------- the step
def test_three_steps_follow_the_float64_gradient_and_move_nothing_else():
    m, ema = grown_model(with_ema=True)
    opt = RowAdamW(m.label_emb.weight, ROWS, lr=1e-2, ema_model=ema, ema_beta=0.9, step_start_ema=2)
    step = TrainStep(m, diffusion(), opt, seed=3)
    before, ema_before = snapshot(m), snapshot(ema)
    ema_rows = []
    for i in range(3):
        ref = gradient64(m)
        prev = m.label_emb.weight.detach()[list(ROWS)].clone()
        loss = call(step)
        g = opt.row_grad.cpu().double()
        err, rn = float((g - ref).norm()), float(ref.norm())
        print(f"call {i}: loss {float(loss):.6f}  ||g - ref|| = {err:.3e}  ||ref|| = {rn:.3e}  relative {err / rn:.2e}")
        assert err < 2e-4 * rn + 1e-7
        now = m.label_emb.weight.detach()[list(ROWS)]
        assert not torch.equal(now, prev), "the rows did not move"
        ema_rows.append((ema.label_emb.weight.detach()[list(ROWS)].clone(), now.clone()))
    assert step.step_index == 3 and opt.step_count == 3 and step._graph is not None
    assert_only_rows_moved(m, before, "model")
    assert_only_rows_moved(ema, ema_before, "EMA model")
    assert all(p.grad is None for p in m.parameters()), "a frozen parameter (or the table) was given a .grad"
    assert m.train_engine._arena is None, "the frozen step carved the gradient arena"
    # EMA rows: plain copy for the first step_start_ema steps, then old * beta + (1 - beta) * new in fp32
    assert torch.equal(ema_rows[0][0], ema_rows[0][1]) and torch.equal(ema_rows[1][0], ema_rows[1][1])
    e_prev, p3 = ema_rows[1][0].cpu().numpy(), ema_rows[2][1].cpu().numpy()
    want = e_prev * np.float32(0.9) + np.float32(1.0 - 0.9) * p3
    assert np.array_equal(ema_rows[2][0].cpu().numpy(), want)


def test_graph_and_eager_give_identical_rows():
    rows = []
    for use_graph in (True, False):
        m = grown_model()
        step = TrainStep(m, diffusion(), RowAdamW(m.label_emb.weight, ROWS, lr=1e-2, weight_decay=0.1, anchor="init"), seed=3,
                         use_graph=use_graph)
        losses = [call(step) for _ in range(3)]
        assert (step._graph is not None) == use_graph
        rows.append((m.label_emb.weight.detach()[list(ROWS)].clone(), torch.cat(losses)))
    assert torch.equal(rows[0][0], rows[1][0]) and torch.equal(rows[0][1], rows[1][1])


def test_masked_min_snr_step_has_the_full_steps_gradient():
    """loss_mask and loss_weights="min_snr": one frozen call leaves the gradient of the full step with the same arguments, at the
    fitted rows, bit for bit (the loss launch is the same one)."""
    m = grown_model()
    mask = torch.rand(B, 1, *HW, generator=torch.Generator().manual_seed(2))
    full = TrainStep(m, diffusion(), FusedAdamW(m.parameters(), lr=0.0), seed=3, loss_weights="min_snr")
    loss_full = call(full, loss_mask=mask)
    want = full.eng.grads()["label_emb.weight"][list(ROWS)].clone()
    sl_full = full.last_sample_losses.clone()
    for p in m.parameters():
        p.grad = None
    opt = RowAdamW(m.label_emb.weight, ROWS, lr=0.0)
    step = TrainStep(m, diffusion(), opt, seed=3, loss_weights="min_snr")
    loss = call(step, loss_mask=mask)
    assert torch.equal(loss, loss_full) and torch.equal(step.last_sample_losses, sl_full)
    assert bool(want.any()) and torch.equal(opt.row_grad.view(torch.int32), want.view(torch.int32))
    assert step._mgraph is not None and step._graph is None


def test_samplers_see_the_fitted_row_and_only_it():
    """A stale derived table would leave the fitted id at its init; an over-written one would move an untouched id."""
    m = grown_model()
    diff, args = diffusion(), make_args(device=DEV)
    X = torch.randn(2, 4, *HW, generator=torch.Generator().manual_seed(8))

    def sample(ids):
        return diff.sampling_ddim(m, None, 2, "fit", torch.tensor(ids, dtype=torch.int64), args, steps=4, eta=0, x_T=X).clone()

    untouched_before, init_before = sample([2, 9]), sample([INIT[0], INIT[1]])
    assert torch.equal(sample(list(ROWS)), init_before), "a new row initialised from a writer must sample as that writer"
    step = TrainStep(m, diffusion(), RowAdamW(m.label_emb.weight, ROWS, lr=5e-2), seed=3)
    for _ in range(3):
        call(step)
    assert torch.equal(sample([2, 9]), untouched_before), "an untouched id samples differently after the fit"
    assert torch.equal(sample([INIT[0], INIT[1]]), init_before)
    assert not torch.equal(sample(list(ROWS)), init_before), "the fitted ids still sample as their init ids"
    # the forward for the new ids against the float64 oracle on the grown, fitted table
    x0, inp, _eps = inputs()
    m.eval()
    with torch.no_grad():
        out = m(x0.to(DEV), timesteps=TS.to(DEV), context=inp["context"].to(DEV), y=inp["y"].to(DEV)).cpu().double()
        ref = oracle(m)[0](x0.double(), TS, inp["context"], inp["y"], None)
    worst = max(max_rel(out[b], ref[b]) for b in range(B))
    print(f"forward with the fitted rows against the oracle: worst per-sample max_rel {worst:.2e}")
    assert worst < 5e-5


def test_refusals_come_before_any_launch(monkeypatch):
    m = grown_model()
    other = grown_model()
    opt = RowAdamW(m.label_emb.weight, ROWS)
    diff = diffusion()
    for kw, msg in ((dict(accumulate=2), "accumulate"), (dict(label_dropout=0.1), "label_dropout"), (dict(bucketed=True), "bucketed")):
        with pytest.raises(ValueError, match=msg):
            TrainStep(m, diff, opt, **kw)
    with pytest.raises(ValueError, match="label_emb.weight"):
        TrainStep(other, diff, opt)
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda group=None: 2)
    monkeypatch.setattr(torch.distributed, "get_rank", lambda group=None: 0)
    with pytest.raises(ValueError, match="world size"):
        TrainStep(m, diff, opt)
    monkeypatch.undo()
    assert m._train_engine is None or not m._train_engine._tplans, "a refused TrainStep built a plan"
    for bad, msg in (((ROWS[0], ROWS[0]), "distinct"), ((m.num_classes,), "lie in"), ((), "1 .. 64")):
        with pytest.raises(ValueError, match=msg):
            RowAdamW(m.label_emb.weight, bad)
    with pytest.raises(ValueError, match="anchor"):
        RowAdamW(m.label_emb.weight, ROWS, anchor=torch.zeros(1, 256))
    with pytest.raises(ValueError, match="ema_model"):
        RowAdamW(m.label_emb.weight, ROWS, ema_model=train_model(SMALL, "base", False, SEEDS[0]))  # (a table that was not grown)


def test_row_adamw_state_dict_round_trip():
    m = grown_model()
    before_rows = m.label_emb.weight.detach()[list(ROWS)].clone()
    opt = RowAdamW(m.label_emb.weight, ROWS, lr=1e-2, anchor="init", weight_decay=0.1)
    step = TrainStep(m, diffusion(), opt, seed=3)
    call(step)
    sd = opt.state_dict()
    assert sd["rows"] == list(ROWS) and sd["step_count"] == 1
    table = m.label_emb.weight.detach().clone()
    call(step)
    want = m.label_emb.weight.detach().clone()
    with torch.no_grad():
        m.label_emb.weight.copy_(table)
    with pytest.raises(ValueError, match="anchor"):
        RowAdamW(m.label_emb.weight, ROWS).load_state_dict(sd)
    opt2 = RowAdamW(m.label_emb.weight, ROWS, lr=1.0, weight_decay=0.5, anchor=torch.zeros(2, 256))
    opt2.load_state_dict(sd)
    assert opt2.step_count == 1 and opt2.lr == 1e-2 and opt2.weight_decay == 0.1 and torch.equal(opt2.exp_avg, sd["exp_avg"])
    assert torch.equal(opt2.anchor, sd["anchor"]) and torch.equal(sd["anchor"], before_rows)
    call(TrainStep(m, diffusion(), opt2, seed=3))
    assert torch.equal(m.label_emb.weight.detach(), want)
    with pytest.raises(ValueError, match="rows"):
        RowAdamW(m.label_emb.weight, ROWS[::-1]).load_state_dict(sd)


# ------------------------------------------------------------------------------------------------------------- the user-facing calls
def test_fit_writers_returns_the_losses_and_counts_the_calls():
    m, ema = grown_model(with_ema=True)
    before, ema_before = snapshot(m), snapshot(ema)
    x0, inp, _eps = inputs()
    lat, ctx = x0[:3].to(DEV), inp["context"][:3]
    losses, step = fit_writers(m, diffusion(), lat, ctx, [ROWS[0], ROWS[0], ROWS[1]], steps=5, batch=2, lr=1e-2, anchor="init",
                               weight_decay=0.01, ema_model=ema, loss_weights="min_snr", loss_mask=torch.ones(*HW), seed=4,
                               return_step=True)
    assert losses.is_cuda and losses.dtype == torch.float32 and tuple(losses.shape) == (5,)
    assert bool(torch.isfinite(losses).all()) and bool((losses > 0).all())
    assert step.step_index == 5 and step.opt.step_count == 5 and step.opt.rows == ROWS
    assert_only_rows_moved(m, before, "model")
    assert_only_rows_moved(ema, ema_before, "EMA model")
    now = m.label_emb.weight.detach()[list(ROWS)]
    assert not torch.equal(now, before["label_emb.weight"][list(ROWS)])
    assert torch.equal(ema.label_emb.weight.detach()[list(ROWS)], now)  # (5 steps < step_start_ema: the warm-up copy)
    again = fit_writers(m, diffusion(), lat, ctx, [ROWS[0], ROWS[0], ROWS[1]], steps=2, batch=3)
    assert tuple(again.shape) == (2,)
    with pytest.raises(ValueError, match="one entry per sample"):
        fit_writers(m, diffusion(), lat, ctx, [ROWS[0]], steps=2, batch=2)


def test_score_writers_is_a_paired_loop_of_eval_loss():
    m = grown_model()
    diff = diffusion()
    x0, inp, _eps = inputs()
    lat, ctx, t = x0[:3].to(DEV), inp["context"][:3], TS[:3]
    cand = [4, 0, ROWS[0], 9, ROWS[1]]  # (ROWS[0] is a copy of writer 4)
    scores = score_writers(m, diff, lat, ctx, cand, t, seed=5, chunk=4)  # 15 (sample, candidate) rows: chunks of 4, 4, 4, 3
    assert scores.is_cuda and scores.dtype == torch.float32 and tuple(scores.shape) == (3, 5)
    # the plain loop: the eps row of every sample drawn once, the rows sample-major, the same chunks
    _, eps = diff.noise_images(lat, t, seed=5)
    pairs = [(s, w) for s in range(3) for w in cand]
    loop = []
    for lo in range(0, len(pairs), 4):
        si = torch.tensor([s for s, _ in pairs[lo:lo + 4]])
        ws = torch.tensor([w for _, w in pairs[lo:lo + 4]])
        loop.append(diff.eval_loss(m, lat[si.to(DEV)], ctx[si], ws, t[si], noise=eps[si.to(DEV)]))
    assert torch.equal(torch.cat(loop).view(3, 5), scores)
    assert torch.equal(scores[:, 0], scores[:, 2]), "two candidates with identical rows must score the same"
    assert not torch.equal(scores[:, 0], scores[:, 1])
    assert int(scores.mean(0).argmin()) in range(len(cand))
    with pytest.raises(ValueError, match="candidate"):
        score_writers(m, diff, lat, ctx, [m.num_classes], t)
