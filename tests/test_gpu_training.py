"""Training gradients of the HIP path against a float64 reference, where the training engine's kernel choices change:

  * ``TrainStep`` (one hipGraph) at the benchmark's training shape: FULL base UNet, B = 64, [4, 8, 32] latents;
  * batches and latent maps at the edges of those choices (a tail sample, a level whose token count is not a multiple of 64,
    the 779-key PHOSC cross-attention at 320 channels), through the reference's call surface (model -> MSELoss -> backward);
  * every switch of ``TrainEngine`` at its non-default value, with the plan showing that the switch took effect;
  * the optimiser kernels (``wd_adamw_multi`` through ``FusedAdamW``, ``wd_mse_loss``) at their chunk and grid edges.

The reference is ``oracle.unet_oracle`` in float64 under torch autograd on the CPU, over the same synthetic weights (every entry
filled, the zero-initialised convolutions too, so that the backward pass is not silenced).  Gradients are held to the bound of
test_gpu_model.py's gradient tests, per parameter: ||g - ref|| < 2e-4 ||ref|| + 1e-7."""
import collections

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests._common import FULL, make_args  # noqa: E402
from tests._train_ref import DEV, case_inputs, check_against_reference, reference64, train_call, train_model  # noqa: E402
from worddiffusion_amd import Diffusion  # noqa: E402


# ------------------------------------------------------------------------------------------ TrainStep at the benchmark shape
def test_train_step_gradients_at_the_benchmark_shape():
    """bench.py's training leg (FULL base, synthetic_inputs(64, seed=7), [4, 8, 32] latents, one hipGraph) with explicit t and
    noise and AdamW at lr 0 without EMA: the update is then exactly p, so the parameters stay put and the gradients stay those
    of the weights the reference sees."""
    from worddiffusion_amd.optim import FusedAdamW
    from worddiffusion_amd.training import TrainStep
    seeds = (0, 7, 11)
    x0, inp, eps = case_inputs(FULL, 64, (8, 32), 0, seeds)
    m = train_model(FULL, "base", False, seeds[0])
    opt = FusedAdamW(m.parameters(), lr=0.0)
    step = TrainStep(m, Diffusion(noise_steps=1000, img_size=(64, 256), args=make_args(device=DEV)), opt, seed=99, use_graph=True)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    args = (x0.to(DEV), inp["context"].to(DEV), inp["y"].to(DEV))
    loss = float(step(*args, t=inp["t"], noise=eps.to(DEV)).cpu())
    torch.cuda.synchronize()
    pred = step._P.out.cpu()
    grads = {k: g.clone() for k, g in step.eng.grads().items()}
    check_against_reference(pred, loss, grads, reference64(FULL, "base", 64, (8, 32), 0, seeds, noised=True),
                            "TrainStep FULL base B=64 (8, 32)")
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), f"{k}: lr = 0 moved the parameter"
    step(*args, t=inp["t"], noise=eps.to(DEV))
    torch.cuda.synchronize()
    again = step.eng.grads()
    assert set(again) == set(grads)
    for k, g in grads.items():
        assert torch.equal(again[k], g), f"{k}: a replayed step changed the gradient"


# ------------------------------------------------------------------------------------------ batches and maps at the edges
@pytest.mark.parametrize("variant,B,hw,phosc_len", [
    ("base", 65, (8, 32), 0),      # a tail sample: M = 16640 at 8 x 32, 4160 at 4 x 16
    ("base", 3, (8, 16), 0),       # the 4 x 8 level has M = 96: weight gradients through transposed planes and wd_gemm
    ("phosc", 8, (8, 32), 769),    # 779-key cross-attention and 256-key self-attention at 320 channels
])
def test_training_gradients_at_the_edges(variant, B, hw, phosc_len):
    seeds = (55, 100 + B, 3)
    x, inp, eps = case_inputs(FULL, B, hw, phosc_len, seeds)
    m = train_model(FULL, variant, phosc_len > 0, seeds[0])
    pred, loss, grads = train_call(m, variant, x, inp, eps, phosc_len)
    check_against_reference(pred, loss, grads, reference64(FULL, variant, B, hw, phosc_len, seeds),
                            f"FULL {variant} B={B} {hw} phosc_len={phosc_len}")


# ------------------------------------------------------------------------------------------ training-engine switches
def plan_facts(P):
    """(launch counts of the backward list, of the forward list, (w_layout, tile) counts of the forward's wd_gemm launches)."""
    bwd = collections.Counter(fn.__name__ for fn, _, _ in P.bwd)
    fwd = collections.Counter(fn.__name__ for fn, _, _ in P.step)
    forms = collections.Counter((a[0]._obj.w_layout, a[0]._obj.tile) for fn, a, _ in P.step if fn.__name__ == "wd_gemm")
    return bwd, fwd, forms


def _default_plan(bwd, fwd, forms):
    # what the switches below turn off or on: all of it is in the default plan at this shape
    assert bwd["wd_dw"] and bwd["wd_dw_group"] and bwd["wd_gn_bwd_fused"] and bwd["wd_dout_prep_geglu"], bwd
    assert bwd["wd_colsum_finish_multi"] and not bwd["wd_gn_bwd_stats"] and not bwd["wd_geglu_bwd"], bwd
    assert forms[(3, 64080)] and not forms[(3, 64320)], forms
    return True


SWITCHES = {
    None: _default_plan,
    ("WDIFF_TRAIN_DW", "0"): lambda b, f, g: not b["wd_dw"] and not b["wd_dw_group"],
    ("WDIFF_DW_GROUP", "1"): lambda b, f, g: not b["wd_dw_group"] and b["wd_dw"],
    ("WDIFF_FUSE_GN_BWD", "0"): lambda b, f, g: (not b["wd_gn_bwd_fused"] and b["wd_gn_bwd_stats"] and
                                                 b["wd_gn_bwd_stats"] == b["wd_gn_bwd_apply"]),
    ("WDIFF_FUSE_GEGLU_BWD", "0"): lambda b, f, g: not b["wd_dout_prep_geglu"] and b["wd_geglu_bwd"],
    ("WDIFF_DEFER_BIAS", "0"): lambda b, f, g: not b["wd_colsum_finish_multi"],
    ("WDIFF_TRAIN_WDIRECT", "1"): lambda b, f, g: g[(3, 64320)] > 0,
    ("WDIFF_TRAIN_SMALLMAP", "0"): lambda b, f, g: not g[(3, 64080)],  # (one forward GEMM at this shape)
}


@pytest.mark.parametrize("switch", list(SWITCHES), ids=lambda s: "default" if s is None else f"{s[0]}={s[1]}")
def test_training_engine_switches(switch, monkeypatch):
    """FULL base, B = 8, 8 x 32 - every switch read in TrainEngine.__init__ changes this shape's plan (checked on the plan) and
    the gradients still meet the float64 reference."""
    for name, _ in filter(None, SWITCHES):
        monkeypatch.delenv(name, raising=False)
    if switch is not None:
        monkeypatch.setenv(*switch)  # (before the model's train_engine exists: the switches are read when it is built)
    seeds = (31, 8, 9)
    x, inp, eps = case_inputs(FULL, 8, (8, 32), 0, seeds)
    m = train_model(FULL, "base", False, seeds[0])
    pred, loss, grads = train_call(m, "base", x, inp, eps, 0)
    plans = list(m.train_engine._tplans.values())
    assert len(plans) == 1
    facts = plan_facts(plans[0])
    assert SWITCHES[switch](*facts), facts
    check_against_reference(pred, loss, grads, reference64(FULL, "base", 8, (8, 32), 0, seeds), f"switch {switch}")


# ------------------------------------------------------------------------------------------ optimiser kernels at their edges
def _close(got, want):
    """element by element: |got - want| <= 1e-6 |want| + 1e-7 max|want|.  (The floor is for elements that cancel to ~0: torch's
    CPU lerp rounds exp_avg + w (g - exp_avg) once, the kernel twice, so from step 2 on m differs in its last place.)"""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    d = (got - want).abs()
    ok = bool((d <= 1e-6 * want.abs() + 1e-7 * float(want.abs().max())).all())
    return ok, float((d / want.abs().clamp_min(1e-30)).max()), torch.equal(got, want)


@pytest.mark.parametrize("ema_mode", [0, 1, 2])
def test_fused_adamw_at_chunk_edges(ema_mode):
    """wd_adamw_multi through FusedAdamW against torch.optim.AdamW(foreach=False) on the CPU, element by element, after steps 1
    and 7: tensors of 1, 8191, 8192, 8193 and 3 * 8192 + 5 elements straddle the chunk of wd_adamw_chunk() and the search for
    the tensor that owns a chunk; one parameter without a gradient keeps p, m and v bit-identical while its EMA still runs
    (ema_mode 0: no EMA, 1: the warm-up copy, 2: the moving average)."""
    from worddiffusion_amd import _native as N
    from worddiffusion_amd.optim import FusedAdamW
    chunk = N.lib().wd_adamw_chunk()
    assert chunk == 8192
    sizes = [1, chunk - 1, chunk, chunk + 1, 3 * chunk + 5, chunk + 1, 7]
    none_at = 5  # this parameter never gets a gradient
    g = torch.Generator().manual_seed(ema_mode)
    init = [torch.randn(n, generator=g) for n in sizes]
    params = [torch.nn.Parameter(v.clone().to(DEV)) for v in init]
    cpu = [torch.nn.Parameter(v.clone()) for v in init]
    ema_init = [torch.randn(n, generator=g) for n in sizes]
    ema = [torch.nn.Parameter(v.clone().to(DEV), requires_grad=False) for v in ema_init]
    ema_ref = [v.clone() for v in ema_init]

    class Holder(torch.nn.Module):
        def __init__(self, ps):
            super().__init__()
            self.ps = torch.nn.ParameterList(ps)

    lr, beta = 1e-3, 0.995
    opt = FusedAdamW(params, lr=lr, ema_model=Holder(ema) if ema_mode else None, ema_beta=beta,
                     step_start_ema=1000 if ema_mode == 1 else 0)
    ref = torch.optim.AdamW(cpu, lr=lr, foreach=False)
    for i, p in enumerate(params):
        if i != none_at:
            p.grad = torch.zeros_like(p)
    report = []
    for step in range(1, 8):
        for i, (p, c) in enumerate(zip(params, cpu)):
            if i != none_at:
                gr = torch.randn(sizes[i], generator=g) * (0.1 * step)
                c.grad = gr.clone()
                p.grad.copy_(gr.to(DEV))  # (the same gradient buffers every step: FusedAdamW keeps its table)
        opt.step()
        ref.step()
        with torch.no_grad():  # EMA.step_ema (train.py:146-170): copy in the warm-up, then old * beta + (1 - beta) * new
            for e, c in zip(ema_ref, cpu):
                e.copy_(c.detach() if ema_mode == 1 else e * beta + (1 - beta) * c.detach())
        torch.cuda.synchronize()
        if step not in (1, 7):
            continue
        for i, (p, c) in enumerate(zip(params, cpu)):
            if i == none_at:
                assert torch.equal(p.detach().cpu(), init[i]) and torch.equal(c.detach(), init[i])
                assert not bool(opt.exp_avg[i].any()) and not bool(opt.exp_avg_sq[i].any()) and not ref.state.get(c)
            else:
                st = ref.state[c]
                for what, got, want in (("p", p, c), ("m", opt.exp_avg[i], st["exp_avg"]), ("v", opt.exp_avg_sq[i], st["exp_avg_sq"])):
                    ok, rel, exact = _close(got, want)
                    report.append((what, step, rel, exact))
                    assert ok, (what, sizes[i], step, rel)
                    assert exact or step > 1 or what == "p", (what, sizes[i], step)  # (step 1: the same roundings as torch)
            if ema_mode:
                ok, rel, exact = _close(ema[i], ema_ref[i])
                report.append(("ema", step, rel, exact))
                assert ok, ("ema", sizes[i], step, rel)
            else:
                assert torch.equal(ema[i].detach().cpu(), ema_init[i])
    worst = collections.defaultdict(lambda: [0.0, True])
    for what, step, rel, exact in report:
        w = worst[(what, step)]
        w[0], w[1] = max(w[0], rel), w[1] and exact
    print("; ".join(f"{what} step {step}: " + ("bit-exact" if ex else f"worst per-element relative error {rel:.1e}")
                    for (what, step), (rel, ex) in sorted(worst.items())))


def test_mse_loss_past_the_block_cap():
    """wd_mse_loss at n = 3 * 262144 + 7: more than 1024 blocks of 256 would be needed, so the grid strides, with a ragged tail."""
    from worddiffusion_amd.optim import mse_loss
    n = 3 * 262144 + 7
    g = torch.Generator().manual_seed(5)
    pred, target = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.5 + 0.25
    loss, grad = mse_loss(pred.to(DEV), target.to(DEV))
    torch.cuda.synchronize()
    d = pred - target
    want = float((d.double() ** 2).sum() / n)
    assert abs(float(loss.cpu()) - want) <= 1e-6 * want
    assert torch.equal(grad.cpu(), torch.tensor(2.0 / n, dtype=torch.float32) * d)
