"""GPU parity of the whole path through the public Python surface (which calls the C-ABI):
UNet forwards against the reference's golden outputs and the oracle, the DDPM trajectory against the reference's
recorded-noise trajectory, and size-independent properties at the benchmark size (B=64).
Tolerance: 1e-3 relative to the fp32 reference (BASELINE.json north_star); the split-bf16 path sits ~1e-5."""
import copy
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ddpm_oracle as D  # noqa: E402
from oracle import unet_oracle as U  # noqa: E402
from tests._common import (DEEP, FULL, FWD_CASES, SMALL, golden_state_dict, load_golden, make_args, max_rel,  # noqa: E402
                           rel_err)
from worddiffusion_amd import EMA, Diffusion, UNetModel, UNetModelPhosc  # noqa: E402
from worddiffusion_amd.synthetic import fill_module_, synthetic_inputs  # noqa: E402

DEV = "cuda:0"
TOL = 1e-3


def build(cfg, variant, phosc_on, sd=None, seed=0):
    args = make_args(device=DEV, phosc=1 if phosc_on else 0)
    cls = UNetModel if variant == "base" else UNetModelPhosc
    m = cls(args=args, **cfg)
    if sd is not None:
        m.load_state_dict(sd, strict=True)
    else:
        fill_module_(m, seed)
    return m.to(DEV).eval()


def call(m, variant, x, t, ctx, y, phosc=None):
    with torch.no_grad():
        if variant == "base":
            return m(x.to(DEV), None, original_images=None, timesteps=t.to(DEV), context=ctx.to(DEV), y=y.to(DEV))
        return m(x.to(DEV), None if phosc is None else phosc.to(DEV), timesteps=t.to(DEV), context=ctx.to(DEV),
                 y=y.to(DEV))


@pytest.mark.parametrize("tag", sorted(FWD_CASES))
def test_forward_matches_reference_golden(golden_dir, tag):
    cfg, variant, phosc_on = FWD_CASES[tag]
    g = load_golden(golden_dir, tag)
    m = build(cfg, variant, phosc_on, golden_state_dict(g))
    phosc = torch.from_numpy(g["phosc"]) if "phosc" in g.files else None
    out = call(m, variant, torch.from_numpy(g["x"]), torch.from_numpy(g["t"]), torch.from_numpy(g["context"]),
               torch.from_numpy(g["y"]), phosc)
    assert out.shape == tuple(g["out"].shape) and out.dtype == torch.float32
    err = max_rel(out.cpu(), g["out"])
    assert err < TOL, (tag, err)
    # the split-bf16 path is expected far inside the tolerance
    assert err < 1e-4, (tag, err)


def test_resample_planes_from_the_producer_epilogue_are_the_split_launch_planes(golden_dir):
    """Downsample / Upsample inputs: operand planes written by the producing GEMM's epilogue (default) vs a wd_split launch
    (engine.fuse_split = False): the same bits, one launch less each."""
    g = load_golden(golden_dir, "fwd_base_full")
    outs, nops = [], []
    for fuse in (True, False):
        m = build(FULL, "base", False, golden_state_dict(g))
        m.engine.fuse_split = fuse
        outs.append(call(m, "base", torch.from_numpy(g["x"]), torch.from_numpy(g["t"]), torch.from_numpy(g["context"]),
                         torch.from_numpy(g["y"])))
        P = next(iter(m.engine._plans.values()))
        nops.append(sum(1 for _, _, what in P.step if what.endswith(":split")))
    assert nops == [0, 2]
    assert torch.equal(outs[0], outs[1])


def test_groupnorm_in_the_combine_launch_equals_the_apply_launch(golden_dir):
    """4x16 level of the full base model: the GroupNorms whose input comes from a K-cut convolution are applied by that GEMM's
    combine launch (wd_gemm_args.gn_*, default) instead of a wd_gn_apply launch (engine.fuse_gn = False).  Same statistics in the
    same summation order, same arithmetic: the outputs agree to rounding of the fused multiply-adds."""
    g = load_golden(golden_dir, "fwd_base_full")
    outs, napply = [], []
    for fuse in (True, False):
        m = build(FULL, "base", False, golden_state_dict(g))
        m.engine.fuse_gn = fuse
        outs.append(call(m, "base", torch.from_numpy(g["x"]), torch.from_numpy(g["t"]), torch.from_numpy(g["context"]),
                         torch.from_numpy(g["y"])))
        P = next(iter(m.engine._plans.values()))
        napply.append(sum(1 for _, _, what in P.step if what.endswith(":apply")))
    assert napply[1] - napply[0] >= 6, napply
    assert max_rel(outs[0].cpu(), outs[1].cpu()) < 2e-6
    assert max_rel(outs[0].cpu(), g["out"]) < 1e-4


def test_two_source_groupnorm_in_one_launch_equals_two_launches(golden_dir):
    """GroupNorm over [h | skip] (decoder ResBlocks): wd_gn_apply2 (default) vs one wd_gn_apply per source (engine.fuse_gn2 = False):
    the same arithmetic per element, the same bits."""
    g = load_golden(golden_dir, "fwd_base_full")
    outs, napply = [], []
    for fuse in (True, False):
        m = build(FULL, "base", False, golden_state_dict(g))
        m.engine.fuse_gn2 = fuse
        m.engine.use_up_phases = False  # (the phase form of the Upsample needs the two-source launch: keep both runs on the 3x3 form)
        outs.append(call(m, "base", torch.from_numpy(g["x"]), torch.from_numpy(g["t"]), torch.from_numpy(g["context"]),
                         torch.from_numpy(g["y"])))
        P = next(iter(m.engine._plans.values()))
        napply.append(sum(1 for _, _, what in P.step if what.endswith(":apply")))
    assert napply[1] - napply[0] == 4, napply
    assert torch.equal(outs[0], outs[1])


def test_forward_blocks_match_oracle_taps(golden_dir):
    """Intermediate activations (every block output) against the oracle on the small config."""
    g = load_golden(golden_dir, "fwd_base_small")
    sd = golden_state_dict(g)
    for variant in ("base", "phosc"):
        keys = {k: v for k, v in sd.items()} if variant == "base" else \
            {k: v for k, v in sd.items() if not k.startswith(("res.", "wrd_proj."))}
        m = build(SMALL, variant, False, keys)
        orc = U.UNetOracle(SMALL, keys, variant, False)
        inp = synthetic_inputs(5, seed=77, hw=(4, 8), num_classes=SMALL["num_classes"])
        taps = {}
        with torch.no_grad():
            ref = orc(inp["x"], inp["t"], inp["context"], inp["y"], None, taps)
        out = call(m, variant, inp["x"], inp["t"], inp["context"], inp["y"])
        assert max_rel(out.cpu(), ref) < 1e-4
        eng = m.engine
        P = eng.plan(5, 4, 8, 10, 0)
        torch.cuda.synchronize()
        # the FiLM table of all ResBlocks and the conditioning context
        ctx = (P.ctx_pl[0].float() + P.ctx_pl[1].float()).cpu().reshape(5, 10, -1)
        assert max_rel(ctx, taps["context"]) < 1e-4


def test_precision_modes(golden_dir):
    g = load_golden(golden_dir, "fwd_base_full")
    m = build(FULL, "base", False, golden_state_dict(g))
    args = [torch.from_numpy(g[k]) for k in ("x", "t", "context", "y")]
    e3 = max_rel(call(m, "base", *args).cpu(), g["out"])
    m.set_precision("bf16")
    e1 = max_rel(call(m, "base", *args).cpu(), g["out"])
    m.set_precision("bf16x3")
    e3b = max_rel(call(m, "base", *args).cpu(), g["out"])
    assert e3 < 1e-4 and e3b == e3          # deterministic, fp32-class
    assert 1e-4 < e1 < 5e-2                   # plain bf16 is NOT inside the 1e-3 parity bar: reported separately


def test_weights_follow_parameter_updates(golden_dir):
    g = load_golden(golden_dir, "fwd_phosc_small_nophosc")
    m = build(SMALL, "phosc", False, golden_state_dict(g))
    args = [torch.from_numpy(g[k]) for k in ("x", "t", "context", "y")]
    o1 = call(m, "phosc", *args)
    with torch.no_grad():
        m.out[2].weight.mul_(2.0)
        m.out[2].bias.mul_(2.0)
    o2 = call(m, "phosc", *args)
    assert max_rel(o2.cpu(), 2 * o1.cpu()) < 1e-5
    m.load_state_dict(golden_state_dict(g))
    assert torch.equal(call(m, "phosc", *args), o1)


def test_ddpm_trajectory_matches_reference(golden_dir):
    g = load_golden(golden_dir, "ddpm_traj")
    T = int(g["T"])
    m = build(SMALL, "phosc", False, seed=int(g["seed"]))
    args = make_args(device=DEV)
    diff = Diffusion(noise_steps=T, img_size=(32, 64), args=args)
    noise = torch.from_numpy(g["noise"])
    rec = []
    labels = torch.from_numpy(g["labels"])

    class IdentityVAE:
        def decode(self, z):
            import types
            return types.SimpleNamespace(sample=z)

    img = diff.sampling(m, IdentityVAE(), 3, str(g["word"]), labels, args, x_T=noise[0], noise=list(noise[1:]),
                        record=rec)
    xs = torch.stack([r.cpu() for r in rec])
    assert xs.shape == tuple(g["x_per_step"].shape)
    assert max_rel(xs, g["x_per_step"]) < 1e-4
    assert float((img - torch.from_numpy(g["image"])).abs().max()) < 1e-3
    # the captured-graph loop gives the same bits as the eager loop
    lat_eager = diff.sampling(m, None, 3, str(g["word"]), labels, args, x_T=noise[0], noise=list(noise[1:]),
                              use_graph=False)
    lat_graph = diff.sampling(m, None, 3, str(g["word"]), labels, args, x_T=noise[0], noise=list(noise[1:]),
                              use_graph=True)
    assert torch.equal(lat_eager, lat_graph)
    assert diff.last_stats["graph"] and diff.last_stats["steps"] == T - 1
    assert Diffusion.sample is Diffusion.sampling


def test_sampling_device_noise_is_shard_invariant():
    """Rank-sharded sampling: sample g's trajectory depends on (seed, g) only."""
    m = build(SMALL, "phosc", False, seed=5)
    args = make_args(device=DEV)
    diff = Diffusion(noise_steps=12, img_size=(32, 64), args=args)
    labels = torch.tensor([1, 2, 3, 4], dtype=torch.int64)
    words = ["MOVE", "text", "a", "Zz"]
    full = diff.sampling(m, None, 4, words, labels, args, seed=99)
    lo = diff.sampling(m, None, 2, words[:2], labels[:2], args, seed=99, sample_offset=0)
    hi = diff.sampling(m, None, 2, words[2:], labels[2:], args, seed=99, sample_offset=2)
    assert max_rel(torch.cat([lo, hi]).cpu(), full.cpu()) < 1e-5
    assert torch.isfinite(full).all() and float(full.std()) > 0.05
    other = diff.sampling(m, None, 4, words, labels, args, seed=100)
    assert not torch.equal(other, full)


def test_noise_images_and_ema_surface():
    args = make_args(device=DEV)
    diff = Diffusion(noise_steps=1000, img_size=(64, 256), args=args)
    x = torch.randn(8, 4, 8, 32, device=DEV)
    t = diff.sample_timesteps(8).to(DEV)
    x_t, eps = diff.noise_images(x, t, seed=3)
    ref = D.noise_images(diff.alpha_hat.cpu(), x.cpu(), t.cpu(), eps.cpu())
    assert torch.equal(x_t.cpu(), ref)
    assert abs(float(eps.mean())) < 0.05 and abs(float(eps.std()) - 1) < 0.05
    m = build(SMALL, "phosc", False, seed=1)
    ema_model = copy.deepcopy(m).eval().requires_grad_(False)
    fill_module_(m, 2)
    m.to(DEV)
    before = {k: v.clone() for k, v in ema_model.state_dict().items()}
    ema = EMA(0.995)
    ema.step = 2000
    ema.step_ema(ema_model, m)
    for (k, p), q in zip(m.named_parameters(), ema_model.parameters()):
        ref = before[k].cpu() * 0.995 + (1 - 0.995) * p.detach().cpu()
        assert float((q.cpu() - ref).abs().max()) <= 2 ** -23 * float(ref.abs().max()) + 1e-12, k
    ema2 = EMA(0.995)
    ema2.step_ema(ema_model, m)  # warm-up: plain copy (train.py:161-170)
    assert all(torch.equal(a, b) for a, b in zip(ema_model.state_dict().values(), m.state_dict().values()))


def test_full_size_properties_b64():
    """BASELINE configs[1] size (B=64, base UNet, 320 channels): determinism, per-sample independence (GroupNorm/LayerNorm/attention
    are per-sample: sample b of the batch == the same sample run alone), and every sample against the oracle (a few seconds of
    CPU at this size)."""
    m = build(FULL, "base", False, seed=0)
    inp = synthetic_inputs(64, seed=2)
    o1 = call(m, "base", inp["x"], inp["t"], inp["context"], inp["y"])
    o2 = call(m, "base", inp["x"], inp["t"], inp["context"], inp["y"])
    assert torch.equal(o1, o2) and torch.isfinite(o1).all()
    for b in (0, 17, 63):
        ob = call(m, "base", inp["x"][b:b + 1], inp["t"][b:b + 1], inp["context"][b:b + 1], inp["y"][b:b + 1])
        # (B=1 and B=64 pick different tiles / k-splits: fp32 summation order differs, nothing else)
        assert max_rel(ob.cpu(), o1[b:b + 1].cpu()) < 5e-5, b
    # ... and all 64 against the oracle itself, sample by sample
    shapes = U.state_dict_shapes(FULL, "base")
    from worddiffusion_amd.synthetic import synthetic_tensor
    sd = {k: torch.from_numpy(synthetic_tensor(k, s, 0)) for k, s in shapes}
    orc = U.UNetOracle(FULL, sd, "base", False)
    with torch.no_grad():
        ref = orc(inp["x"], inp["t"], inp["context"], inp["y"])
    out = o1.cpu()
    errs = [max_rel(out[b], ref[b]) for b in range(64)]
    assert max(errs) < 1e-4, [(b, e) for b, e in enumerate(errs) if e >= 1e-4]


def test_upsample_as_four_phases_equals_the_nine_tap_form():
    """Upsample (nearest x2 + conv3x3, unet.py:488-499) at the benchmark batch: four 2x2 convolutions of the source map with summed
    taps, phase-major rows read back by the decoder block's GroupNorm (engine.use_up_phases, default) vs the 9-tap gather form -
    the same sums in a different association."""
    inp = synthetic_inputs(64, seed=3)
    outs = []
    for phases in (True, False):
        m = build(FULL, "base", False, seed=1)
        m.engine.use_up_phases = phases
        outs.append(call(m, "base", inp["x"], inp["t"], inp["context"], inp["y"]))
        P = next(iter(m.engine._plans.values()))
        assert sum(1 for _, _, what in P.step if "4 phases" in what) == (1 if phases else 0)
    assert torch.isfinite(outs[0]).all() and max_rel(outs[0].cpu(), outs[1].cpu()) < 2e-5


def test_weights_change_after_a_phase_major_upsample_plan():
    """A parameter update after the phase plan exists (EMA sampling during training): refresh_weights re-derives the summed-tap
    tensor, repacks the four phase matrices from its pieces (column offset t * cin) and writes the grouped fragment-major images
    in the same launch.  B = 64 is the smallest batch whose plan holds the phase launch: its 4 B tiles of 64 rows must fill the
    256 CUs (engine.wdirect_fills_chip)."""
    from worddiffusion_amd.engine import wdirect_fills_chip
    B, scale = 64, 1.25
    assert wdirect_fills_chip(B * 4 * 64, 320) and not wdirect_fills_chip((B - 1) * 4 * 64, 320)
    inp = synthetic_inputs(B, seed=3)
    m = build(FULL, "base", False, seed=1)
    eng = m.engine
    assert eng.use_up_phases
    before = call(m, "base", inp["x"], inp["t"], inp["context"], inp["y"])
    P = next(iter(eng._plans.values()))
    assert sum(1 for _, _, what in P.step if "4 phases" in what) == 1
    names = sorted(k for k in eng._wf if ".wph" in k)
    assert len(names) == 4 and all(n in eng._w for n in names)
    old = {n: eng._wf[n].clone() for n in names}
    with torch.no_grad():
        for p_ in m.parameters():
            p_.mul_(scale)
    eng.refresh_weights()
    assert eng._pack[4] == []
    st = torch.cuda.current_stream(DEV).cuda_stream
    for n in names:
        want = torch.empty(eng._wf[n].shape, dtype=torch.bfloat16, device=DEV)
        eng._pack_wf(n, want, st)
        torch.cuda.synchronize()
        assert torch.equal(eng._wf[n], want), n
        assert not torch.equal(eng._wf[n], old[n]), n
    after = call(m, "base", inp["x"], inp["t"], inp["context"], inp["y"])
    assert next(iter(eng._plans.values())) is P  # the plan built before the update ran again
    fresh = build(FULL, "base", False, seed=1)
    fresh.engine.use_up_phases = False
    with torch.no_grad():
        for p_ in fresh.parameters():
            p_.mul_(scale)
    ref = call(fresh, "base", inp["x"], inp["t"], inp["context"], inp["y"])
    assert all("4 phases" not in what for _, _, what in next(iter(fresh.engine._plans.values())).step)
    assert torch.isfinite(after).all() and not torch.equal(after, before)
    assert max_rel(after.cpu(), ref.cpu()) < 2e-5


def test_full_size_properties_b64_phosc():
    """BASELINE configs[4]'s one-GPU share at the benchmark batch: UNetModelPhosc (args.phosc = 1), 320 channels, 10 word ids +
    the 769-int PHOSC vector (779-key cross-attention, 256-key self-attention), B = 64 - determinism, per-sample independence
    (sample b of the batch == the same sample run alone) and every sample against the oracle."""
    m = build(FULL, "phosc", True, seed=0)
    inp = synthetic_inputs(64, seed=4, phosc_len=769)
    o1 = call(m, "phosc", inp["x"], inp["t"], inp["context"], inp["y"], inp["phosc"])
    o2 = call(m, "phosc", inp["x"], inp["t"], inp["context"], inp["y"], inp["phosc"])
    assert o1.shape == (64, 4, 8, 32) and torch.equal(o1, o2) and torch.isfinite(o1).all()
    for b in (0, 33, 63):
        ob = call(m, "phosc", inp["x"][b:b + 1], inp["t"][b:b + 1], inp["context"][b:b + 1], inp["y"][b:b + 1], inp["phosc"][b:b + 1])
        assert max_rel(ob.cpu(), o1[b:b + 1].cpu()) < 5e-5, b
    shapes = U.state_dict_shapes(FULL, "phosc")
    from worddiffusion_amd.synthetic import synthetic_tensor
    sd = {k: torch.from_numpy(synthetic_tensor(k, s, 0)) for k, s in shapes}
    orc = U.UNetOracle(FULL, sd, "phosc", True)
    with torch.no_grad():
        ref = orc(inp["x"], inp["t"], inp["context"], inp["y"], inp["phosc"])
    out = o1.cpu()
    errs = [max_rel(out[b], ref[b]) for b in range(64)]
    assert max(errs) < 1e-4, [(b, e) for b, e in enumerate(errs) if e >= 1e-4]


def test_optimizer_side_of_train_step(golden_dir):
    """MSE loss / gradient and the fused AdamW(+EMA) launch against the reference's own train step
    (tests/golden/train_step.npz: loss, AdamW-updated tensors) and torch.optim.AdamW semantics."""
    from worddiffusion_amd.optim import FusedAdamW, mse_loss
    from worddiffusion_amd.synthetic import synthetic_tensor
    g = load_golden(golden_dir, "train_step")
    pred, eps = torch.from_numpy(g["pred"]).to(DEV), torch.from_numpy(g["eps"]).to(DEV)
    loss, grad = mse_loss(pred, eps)
    assert abs(float(loss.item()) - float(g["loss"])) < 1e-6
    ref_grad = 2 * (pred - eps) / pred.numel()
    assert max_rel(grad.cpu(), ref_grad.cpu()) < 1e-6
    # AdamW step 1 with the reference's gradients on the four tensors the golden file carries
    keys = [n[6:] for n in g.files if n.startswith("adamw:")]
    shapes = dict(U.state_dict_shapes(SMALL, "phosc"))
    params = [torch.nn.Parameter(torch.from_numpy(synthetic_tensor(k, shapes[k], int(g["seed_model"]))).to(DEV)) for k in keys]
    for p, k in zip(params, keys):
        p.grad = torch.from_numpy(g["grad:" + k]).to(DEV)
    ema_params = [torch.nn.Parameter(torch.zeros_like(p)) for p in params]

    class Holder(torch.nn.Module):
        def __init__(self, ps):
            super().__init__()
            self.ps = torch.nn.ParameterList(ps)

    opt = FusedAdamW(params, lr=1e-4, ema_model=Holder(ema_params), ema_beta=0.995, step_start_ema=1)
    opt.step()
    for p, e, k in zip(params, ema_params, keys):
        assert max_rel(p.detach().cpu(), g["adamw:" + k]) < 1e-6, k
        assert torch.equal(e.detach(), p.detach())  # warm-up step: plain copy
    # second step against torch.optim.AdamW on the CPU, EMA now averaging
    cpu = [torch.nn.Parameter(torch.from_numpy(synthetic_tensor(k, shapes[k], int(g["seed_model"])))) for k in keys]
    ref_opt = torch.optim.AdamW(cpu, lr=1e-4)
    for step in range(2):
        for c, p, k in zip(cpu, params, keys):
            gr = torch.from_numpy(g["grad:" + k]) * (1.0 + step)
            c.grad = gr.clone()
            p.grad.copy_(gr.to(DEV))
        ref_opt.step()
        if step == 1:
            before = [e.detach().clone() for e in ema_params]
            opt.step()
    for c, p, e, b in zip(cpu, params, ema_params, before):
        assert max_rel(p.detach().cpu(), c.detach()) < 1e-6
        ref_e = b.cpu() * 0.995 + (1 - 0.995) * p.detach().cpu()
        assert max_rel(e.detach().cpu(), ref_e) < 1e-6


def _oracle_train_reference(cfg, seed, inp, eps):
    """Oracle forward + autograd on the CPU (fp32): loss, prediction and every parameter gradient."""
    from worddiffusion_amd.synthetic import synthetic_tensor
    shapes = U.state_dict_shapes(cfg, "base")
    sd = {k: torch.from_numpy(synthetic_tensor(k, s, seed)).requires_grad_(True) for k, s in shapes}
    # zero-initialised convolutions (out, proj_out, out_layers.3) would silence most of the backward: they are filled too
    orc = U.UNetOracle(cfg, sd, "base", False)
    pred = orc(inp["x"], inp["t"], inp["context"], inp["y"])
    loss = torch.nn.functional.mse_loss(pred, eps)
    loss.backward()
    return sd, pred.detach(), loss.detach()


@pytest.mark.parametrize("cfg_name,B,hw", [("SMALL", 4, (4, 8)), ("DEEP", 3, (8, 16)), ("SMALL", 2, (8, 32)), ("FULL", 2, (8, 32))])
def test_training_step_gradients_match_oracle_autograd(cfg_name, B, hw):
    """model(...) in train mode -> MSELoss -> loss.backward() (train.py:287-291) on the HIP path vs the oracle under torch
    autograd: loss, prediction and EVERY parameter gradient (and the same set of parameters left without a gradient)."""
    cfg = {"SMALL": SMALL, "DEEP": DEEP, "FULL": FULL}[cfg_name]
    seed = 77
    inp = synthetic_inputs(B, seed=43, hw=hw, num_classes=cfg["num_classes"])
    eps = torch.from_numpy(np.random.RandomState(44).standard_normal(tuple(inp["x"].shape)).astype(np.float32))
    sd, pred_ref, loss_ref = _oracle_train_reference(cfg, seed, inp, eps)
    m = UNetModel(args=make_args(), **cfg)
    fill_module_(m, seed)
    m = m.to(DEV).train()
    pred = m(inp["x"].to(DEV), timesteps=inp["t"].to(DEV), context=inp["context"].to(DEV), y=inp["y"].to(DEV))
    assert pred.requires_grad
    loss = torch.nn.MSELoss()(eps.to(DEV), pred)
    loss.backward()
    torch.cuda.synchronize()
    assert max_rel(pred.detach().cpu(), pred_ref) < 5e-5
    assert abs(float(loss.detach()) - float(loss_ref)) < 1e-5 * max(1.0, float(loss_ref))
    params = dict(m.named_parameters())
    worst = ("", 0.0)
    for k, ref in sd.items():
        g = params[k].grad
        if ref.grad is None:
            assert g is None, f"{k}: the reference leaves this parameter without a gradient"
            continue
        assert g is not None, f"{k}: missing gradient"
        assert tuple(g.shape) == tuple(ref.grad.shape), k
        r = ref.grad.double()
        err = float((g.detach().cpu().double() - r).norm())
        tol = 2e-4 * float(r.norm()) + 1e-7  # (a few gradients are analytically ~0: absolute floor)
        if err / (float(r.norm()) + 1e-30) > worst[1] and float(r.norm()) > 1e-6:
            worst = (k, err / float(r.norm()))
        assert err < tol, (k, err, float(r.norm()))
    print("worst relative gradient error:", worst)
    # a second backward after zero_grad reproduces the gradients bit for bit (deterministic reductions)
    g1 = {k: p.grad.clone() for k, p in params.items() if p.grad is not None}
    for p in m.parameters():
        p.grad = None
    pred2 = m(inp["x"].to(DEV), timesteps=inp["t"].to(DEV), context=inp["context"].to(DEV), y=inp["y"].to(DEV))
    torch.nn.MSELoss()(eps.to(DEV), pred2).backward()
    torch.cuda.synchronize()
    for k, g in g1.items():
        assert torch.equal(params[k].grad, g), k
    # keeping .grad (no zero_grad) accumulates like autograd
    pred3 = m(inp["x"].to(DEV), timesteps=inp["t"].to(DEV), context=inp["context"].to(DEV), y=inp["y"].to(DEV))
    torch.nn.MSELoss()(eps.to(DEV), pred3).backward()
    torch.cuda.synchronize()
    k0 = "input_blocks.1.0.in_layers.2.weight"
    assert max_rel(params[k0].grad, 2 * g1[k0]) < 1e-6


@pytest.mark.parametrize("variant,train", [("base", False), ("phosc", False), ("base", True)])
def test_device_repack_equals_host_specification(variant, train):
    """wd_repack_multi (one launch for every operand) against _Recipe.host(): the split-bf16 planes must be exactly
    split(host matrix) and the fp32 vectors bit-identical; a parameter update is picked up by the next refresh."""
    m = build(DEEP, variant, variant == "phosc", seed=5)
    eng = m.train_engine if train else m.engine
    eng.refresh_weights()
    torch.cuda.synchronize()
    book = eng._recipes()
    assert len(book) > 50
    for name, r in book.items():
        want = r.host()
        got = eng._w[name]
        if r.planes:
            hi = want.to(torch.bfloat16)
            lo = (want - hi.float()).to(torch.bfloat16)
            assert torch.equal(got[0], hi) and torch.equal(got[1], lo), name
        else:
            assert torch.equal(got, want), name
    with torch.no_grad():
        m.out[2].weight.mul_(1.5)
        m.input_blocks[1][0].in_layers[2].bias.add_(0.25)
    eng.refresh_weights()
    torch.cuda.synchronize()
    for name in ("out.w", "in1.0.c1.b"):
        want = eng._recipes()[name].host()
        got = eng._w[name]
        assert torch.equal(got[0], want.to(torch.bfloat16)) if got.dtype == torch.bfloat16 else torch.equal(got, want), name


def test_device_repack_writes_the_fragment_major_images_itself():
    """The fragment-major weight images (wd_gemm_pack_w's layout, read by the weights-to-registers kernels) come out of the same
    wd_repack_multi launch (mode 3) after a parameter update: bit-identical to packing the refreshed planes."""
    m = build(DEEP, "base", False, seed=6)
    eng = m.engine
    eng.refresh_weights()
    book = eng._recipes()
    names = [n for n, r in book.items() if book.frag_ok(r)]
    kinds = {tuple(sorted({(pc[5], pc[6] > 0, pc[7] > 0, pc[9] > 0) for pc in book[n].pieces})) for n in names}
    assert len(names) > 20 and len(kinds) >= 3  # 3x3 and 1x1 pieces, pieces at a column offset, GEGLU-interleaved rows
    for n in names:
        eng._wfrag(n)
    with torch.no_grad():
        for p_ in m.parameters():
            p_.mul_(1.25)
    eng.refresh_weights()
    assert eng._pack[4] == []
    st = torch.cuda.current_stream(DEV).cuda_stream
    for n in names:
        want = torch.empty_like(eng._wf[n])
        eng._pack_wf(n, want, st)
        torch.cuda.synchronize()
        assert torch.equal(eng._wf[n], want), n


def _make_train_setup(cfg, seed, ema=True, **kw):
    from worddiffusion_amd.optim import FusedAdamW
    from worddiffusion_amd.training import TrainStep
    m = UNetModel(args=make_args(device=DEV), **cfg)
    fill_module_(m, seed)
    m = m.to(DEV).train()
    ema_m = copy.deepcopy(m).eval().requires_grad_(False) if ema else None
    opt = FusedAdamW(m.parameters(), lr=1e-4, ema_model=ema_m, ema_beta=0.995, step_start_ema=1)
    diff = Diffusion(noise_steps=1000, img_size=(32, 64), args=make_args(device=DEV))
    return m, ema_m, opt, TrainStep(m, diff, opt, seed=3, **kw)


def test_train_step_loop_matches_oracle_loop():
    """Three iterations of the train.py batch loop (noise_images -> model -> MSE -> backward -> AdamW -> EMA) through
    TrainStep (one hipGraph + optimiser + repack per step) against the same loop on the CPU: oracle forward under torch
    autograd + torch.optim.AdamW + the reference EMA rule.  Then: graph replay == eager launches, bit for bit."""
    from worddiffusion_amd.synthetic import synthetic_tensor
    cfg, seed, B, hw = SMALL, 91, 4, (4, 8)
    steps = 3
    rs = np.random.RandomState(5)
    batches = []
    for i in range(steps):
        inp = synthetic_inputs(B, seed=100 + i, hw=hw, num_classes=cfg["num_classes"])
        inp["t"] = torch.from_numpy(rs.randint(1, 1000, size=(B,))).long()
        inp["eps"] = torch.from_numpy(rs.standard_normal(tuple(inp["x"].shape)).astype(np.float32))
        batches.append(inp)
    # ---- CPU loop
    shapes = U.state_dict_shapes(cfg, "base")
    sd = {k: torch.from_numpy(synthetic_tensor(k, s, seed)).requires_grad_(True) for k, s in shapes}
    init = {k: v.detach().clone() for k, v in sd.items()}
    ema_sd = {k: v.detach().clone() for k, v in sd.items()}
    orc = U.UNetOracle(cfg, sd, "base", False)
    topt = torch.optim.AdamW(list(sd.values()), lr=1e-4)
    _, _, ah = D.schedule(1000)
    ref_losses = []
    for i, b in enumerate(batches):
        x_t = D.noise_images(ah, b["x"], b["t"], b["eps"])
        loss = torch.nn.functional.mse_loss(orc(x_t, b["t"], b["context"], b["y"]), b["eps"])
        topt.zero_grad()
        loss.backward()
        topt.step()
        ref_losses.append(float(loss.detach()))
        with torch.no_grad():  # EMA.step_ema with step_start_ema=1: copy on the first call, then the average
            for k in sd:
                ema_sd[k] = sd[k].detach().clone() if i < 1 else ema_sd[k] * 0.995 + (1 - 0.995) * sd[k].detach()
    # ---- HIP loop (graph) and the same again with eager launches
    results = []
    for use_graph in (True, False):
        m, ema_m, opt, step = _make_train_setup(cfg, seed, use_graph=use_graph)
        losses = []
        for b in batches:
            loss = step(b["x"].to(DEV), b["context"].to(DEV), b["y"].to(DEV), t=b["t"], noise=b["eps"].to(DEV))
            losses.append(float(loss.cpu()))
        torch.cuda.synchronize()
        results.append((losses, {k: v.detach().cpu() for k, v in m.state_dict().items()},
                        {k: v.detach().cpu() for k, v in ema_m.state_dict().items()}))
    (losses, params, ema_params), (losses_e, params_e, ema_e) = results
    assert losses == losses_e
    for k in params:
        assert torch.equal(params[k], params_e[k]) and torch.equal(ema_params[k], ema_e[k]), k
    for a, r in zip(losses, ref_losses):
        assert abs(a - r) < 2e-4 * max(1.0, abs(r)), (losses, ref_losses)
    worst = 0.0
    for k, v in sd.items():
        upd = (v.detach() - init[k]).double()
        if sd[k].grad is None:
            assert torch.equal(params[k], init[k]), f"{k}: no gradient in the reference -> AdamW leaves it untouched"
            continue
        if upd.numel() < 256:
            continue
        # Adam's first steps move every coordinate by ~lr * sign(g): coordinates whose gradient is numerically ~0 may
        # flip, so the comparison is on the update as a whole (norm), not per element
        rel = float((params[k].double() - v.detach().double()).norm() / (upd.norm() + 1e-30))
        worst = max(worst, rel)
        assert rel < 0.05, (k, rel)
        erel = float((ema_params[k].double() - ema_sd[k].double()).norm() / ((ema_sd[k] - init[k]).double().norm() + 1e-30))
        assert erel < 0.05, (k, erel)
    print("worst relative update error:", worst)


def test_train_step_device_noise_and_timesteps():
    """Without explicit t / noise the step draws t on the host (train.py:281) and eps from the device Philox stream;
    the loss is finite and decreases on a fixed batch over a few dozen steps."""
    m, ema_m, opt, step = _make_train_setup(SMALL, 7, ema=False)
    inp = synthetic_inputs(8, seed=1, hw=(4, 8), num_classes=SMALL["num_classes"])
    x, c, y = inp["x"].to(DEV), inp["context"].to(DEV), inp["y"].to(DEV)
    t = torch.full((8,), 500, dtype=torch.int64)
    eps = torch.randn(x.shape, generator=torch.Generator().manual_seed(0)).to(DEV)
    first = float(step(x, c, y, t=t, noise=eps).cpu())
    for _ in range(40):
        last = float(step(x, c, y, t=t, noise=eps).cpu())
    assert np.isfinite(last) and last < 0.7 * first, (first, last)
    l2 = float(step(x, c, y).cpu())
    assert np.isfinite(l2)


def test_train_step_matches_reference_golden(golden_dir):
    """The reference's own train step (tests/golden/train_step.npz: train.py:287-294 run on UNetModelPhosc with MSELoss,
    loss.backward(), AdamW(lr 1e-4), EMA) against the HIP path: prediction, loss, the recorded gradients (convs, attention
    projections, GEGLU, embeddings, word-encoder), the AdamW-updated tensors."""
    from worddiffusion_amd.optim import FusedAdamW
    g = load_golden(golden_dir, "train_step")
    m = UNetModelPhosc(args=make_args(device=DEV), **SMALL)
    fill_module_(m, int(g["seed_model"]))
    m = m.to(DEV).train()
    opt = FusedAdamW(m.parameters(), lr=1e-4)
    pred = m(torch.from_numpy(g["x_t"]).to(DEV), None, timesteps=torch.from_numpy(g["t"]).to(DEV),
             context=torch.from_numpy(g["context"]).to(DEV), y=torch.from_numpy(g["y"]).to(DEV))
    loss = torch.nn.MSELoss()(torch.from_numpy(g["eps"]).to(DEV), pred)
    opt.zero_grad()
    loss.backward()
    torch.cuda.synchronize()
    assert max_rel(pred.detach().cpu(), g["pred"]) < 5e-5
    assert abs(float(loss.detach()) - float(g["loss"])) < 1e-5
    params = dict(m.named_parameters())
    gsq = 0.0
    for k, p in params.items():
        if p.grad is not None:
            gsq += float((p.grad.double() ** 2).sum())
    assert abs(gsq ** 0.5 - float(g["grad_norm"])) < 2e-4 * float(g["grad_norm"])
    for name in g.files:
        if name.startswith("grad:"):
            k = name[5:]
            ref = torch.from_numpy(g[name]).double()
            err = float((params[k].grad.detach().cpu().double() - ref).norm())
            assert err < 2e-4 * float(ref.norm()) + 1e-7, (k, err, float(ref.norm()))
    opt.step()
    torch.cuda.synchronize()
    for name in g.files:
        if name.startswith("adamw:"):
            k = name[6:]
            # first Adam step: +-lr per coordinate; coordinates with |g| ~ 1e-8 may differ in sign -> norm-wise check
            ref = torch.from_numpy(g[name]).double()
            got = params[k].detach().cpu().double()
            assert float((got - ref).norm()) < 0.02 * 1e-4 * ref.numel() ** 0.5, k


@pytest.mark.parametrize("cfg_name,B,hw,phosc_len", [("SMALL", 2, (4, 8), 769), ("DEEP", 2, (8, 16), 40), ("FULL", 1, (8, 32), 0)])
def test_phosc_training_gradients_match_oracle_autograd(cfg_name, B, hw, phosc_len):
    """UNetModelPhosc train step (spatial self-attention, PHOSC tokens in the context) vs oracle autograd, all gradients."""
    from worddiffusion_amd.synthetic import synthetic_tensor
    cfg = {"SMALL": SMALL, "DEEP": DEEP, "FULL": FULL}[cfg_name]
    seed = 55
    inp = synthetic_inputs(B, seed=21, hw=hw, num_classes=cfg["num_classes"], phosc_len=phosc_len)
    eps = torch.from_numpy(np.random.RandomState(3).standard_normal(tuple(inp["x"].shape)).astype(np.float32))
    shapes = U.state_dict_shapes(cfg, "phosc")
    sd = {k: torch.from_numpy(synthetic_tensor(k, s, seed)).requires_grad_(True) for k, s in shapes}
    orc = U.UNetOracle(cfg, sd, "phosc", phosc_len > 0)
    pred_ref = orc(inp["x"], inp["t"], inp["context"], inp["y"], inp.get("phosc"))
    torch.nn.functional.mse_loss(pred_ref, eps).backward()
    m = UNetModelPhosc(args=make_args(device=DEV, phosc=1 if phosc_len else 0), **cfg)
    fill_module_(m, seed)
    m = m.to(DEV).train()
    pred = m(inp["x"].to(DEV), inp["phosc"].to(DEV) if phosc_len else None, timesteps=inp["t"].to(DEV),
             context=inp["context"].to(DEV), y=inp["y"].to(DEV))
    torch.nn.MSELoss()(eps.to(DEV), pred).backward()
    torch.cuda.synchronize()
    assert max_rel(pred.detach().cpu(), pred_ref.detach()) < 5e-5
    params = dict(m.named_parameters())
    for k, ref in sd.items():
        gr = params[k].grad
        if ref.grad is None:
            assert gr is None, k
            continue
        assert gr is not None, k
        r = ref.grad.double()
        err = float((gr.detach().cpu().double() - r).norm())
        assert err < 2e-4 * float(r.norm()) + 1e-7, (k, err, float(r.norm()))


def test_step_skipping_sampler_and_bulk_driver(tmp_path):
    """Diffusion.sampling3 (regenerateFromtrain2.py:465-648: predicted noise refreshed 1 step in 5, deterministic update)
    against the oracle's restatement of that loop; then the bulk driver: rows sharded over 2 "ranks" and small batches give
    the same latents as one big call (global-row-indexed noise)."""
    from worddiffusion_amd.driver import regenerate, writer_dict
    T = 23
    m = build(SMALL, "base", False, seed=3)
    args = make_args(device=DEV)
    args.fullSampling = False
    diff = Diffusion(noise_steps=T, img_size=(32, 64), args=args)
    words = ["MOVE", "a", "Zebra"]
    labels = torch.tensor([1, 4, 7], dtype=torch.int64)
    x_t = torch.randn(3, 4, 4, 8, generator=torch.Generator().manual_seed(8))
    got = diff.sampling3(0, x_t.to(DEV), words, None, m, m, None, 0, 0, 3, words, labels.to(DEV), args)
    assert diff.last_stats["model_calls"] == len([i for i in range(1, T) if i % 5 == 0 or i == T - 1])
    # oracle loop on the CPU
    shapes = U.state_dict_shapes(SMALL, "base")
    from worddiffusion_amd.synthetic import synthetic_tensor
    sd = {k: torch.from_numpy(synthetic_tensor(k, s, 3)) for k, s in shapes}
    orc = U.UNetOracle(SMALL, sd, "base", False)
    tf = torch.tensor(np.array([D.label_padding(w) for w in words], dtype="int64"))
    with torch.no_grad():
        ref, calls = D.sampling3(lambda x, t: orc(x, t, tf, labels), x_t, T)
    assert calls == diff.last_stats["model_calls"]
    assert max_rel(got.cpu(), ref) < 2e-4
    # ---- bulk driver: 5 rows, batch 2, two ranks == one call over all rows
    rows = [("w1", "img0", "MOVE"), ("w2", "img1", "to"), ("w1", "img2", "a"), ("w3", "img3", "Stop"), ("w2", "img4", "it")]
    wr = writer_dict(rows)
    diff2 = Diffusion(noise_steps=9, img_size=(32, 64), args=args)
    _, whole = regenerate(m, diff2, rows, wr, args, batch=8, seed=5, rank=0, world=1)
    parts = []
    for r in range(2):
        s0, part = regenerate(m, diff2, rows, wr, args, batch=2, seed=5, rank=r, world=2, out_dir=str(tmp_path))
        parts.append(part)
    assert max_rel(torch.cat(parts), whole) < 1e-5
    assert sorted(os.listdir(tmp_path)) == [f"img{i}.npy" for i in range(5)]
    assert np.allclose(np.load(tmp_path / "img3.npy"), whole[3].numpy(), atol=1e-5)


def test_training_in_single_pass_bf16_mode():
    """set_precision('bf16') (single MFMA pass, fp32 master weights / accumulation) also drives the training plan: gradients
    agree with the split-bf16 ones to bf16 accuracy (a few 1e-2) - reported separately from the parity mode."""
    cfg, B, hw = SMALL, 4, (8, 32)
    inp = synthetic_inputs(B, seed=43, hw=hw, num_classes=cfg["num_classes"])
    eps = torch.from_numpy(np.random.RandomState(44).standard_normal(tuple(inp["x"].shape)).astype(np.float32)).to(DEV)
    m = UNetModel(args=make_args(device=DEV), **cfg)
    fill_module_(m, 12)
    m = m.to(DEV).train()
    args = dict(timesteps=inp["t"].to(DEV), context=inp["context"].to(DEV), y=inp["y"].to(DEV))
    grads = {}
    for mode in ("bf16x3", "bf16"):
        m.set_precision(mode)
        for p in m.parameters():
            p.grad = None
        torch.nn.MSELoss()(eps, m(inp["x"].to(DEV), **args)).backward()
        torch.cuda.synchronize()
        grads[mode] = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    m.set_precision("bf16x3")
    worst = 0.0
    for k, g in grads["bf16x3"].items():
        if g.numel() < 64 or float(g.norm()) < 1e-6:
            continue
        worst = max(worst, rel_err(grads["bf16"][k].cpu(), g.cpu()))
    assert 1e-4 < worst < 0.15, worst


@pytest.mark.parametrize("cfg_name,variant,B,hw,phosc_len", [("FULL", "base", 1, (8, 32), 0), ("FULL", "base", 3, (8, 16), 0),
                                                              ("FULL", "base", 5, (4, 8), 0), ("SMALL", "base", 65, (8, 32), 0),
                                                              ("FULL", "phosc", 2, (8, 16), 769), ("DEEP", "phosc", 3, (8, 32), 5),
                                                              ("SMALL", "base", 2, (2, 4), 0)])
def test_forward_ragged_shapes_match_oracle(cfg_name, variant, B, hw, phosc_len):
    """Batch sizes and latent sizes away from the benchmark shape (tails of the 128-row GEMM panels, of the 32-token folded
    attention tiles, of the GroupNorm chunks; 64x128 and 32x64 images; a 65-sample batch) against the oracle."""
    cfg = {"SMALL": SMALL, "DEEP": DEEP, "FULL": FULL}[cfg_name]
    from worddiffusion_amd.synthetic import synthetic_tensor
    seed = 17
    shapes = U.state_dict_shapes(cfg, variant)
    sd = {k: torch.from_numpy(synthetic_tensor(k, s, seed)) for k, s in shapes}
    orc = U.UNetOracle(cfg, sd, variant, phosc_len > 0)
    inp = synthetic_inputs(B, seed=B * 7 + hw[1], hw=hw, num_classes=cfg["num_classes"], phosc_len=phosc_len)
    with torch.no_grad():
        ref = orc(inp["x"], inp["t"], inp["context"], inp["y"], inp.get("phosc"))
    m = build(cfg, variant, phosc_len > 0, seed=seed)
    out = call(m, variant, inp["x"], inp["t"], inp["context"], inp["y"], inp.get("phosc"))
    assert out.shape == ref.shape
    assert max_rel(out.cpu(), ref) < 1e-4
    # and through the sampler (tabulated FiLM path, folded attention, graph): 3 steps from the same start
    if variant == "base" and B <= 5:
        T = 4
        args = make_args(device=DEV)
        diff = Diffusion(noise_steps=T, img_size=(hw[0] * 8, hw[1] * 8), args=args)
        words = ["ab", "Word", "x", "Hello", "zz"][:B]
        tf = torch.tensor(np.array([D.label_padding(w) for w in words], dtype="int64"))
        noise = [torch.randn(B, 4, *hw, generator=torch.Generator().manual_seed(i)) for i in range(T - 2)]
        got = diff.sampling(m, None, B, words, inp["y"], args, x_T=inp["x"], noise=noise)
        with torch.no_grad():
            want = D.sampling(lambda x, t: orc(x, t, tf, inp["y"]), inp["x"], noise, T)
        assert max_rel(got.cpu(), want) < 2e-4
