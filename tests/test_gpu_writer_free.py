"""Writer-free guidance on the GPU, model and samplers: the ``writer_keep`` forwards and the guided DDPM loop against what the
reference's own modules computed (``tests/golden/writer_free.npz``, ``tools/make_golden_writer_free.py``), the autograd call with
a mixed mask against the float64 oracle, guided DDIM / DPM-Solver++ against their host specifications, graph replay against
eager launches, and that nothing changes for a call without the new arguments.

Bars: 1e-4 max-norm relative for a forward and for the states of a short trajectory (``tests/test_gpu_interp.py``);
(|s| + |1 - s|) 1e-4 for the guided prediction; 1e-3 absolute for the image; the training bounds of
``tests/test_gpu_dropout.check_against_reference``."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ddpm_oracle as D  # noqa: E402
from oracle import unet_oracle as U  # noqa: E402
from tests import _ddim_ref as DDIM  # noqa: E402
from tests import _dpmpp_ref as DPM  # noqa: E402
from tests import _labeldrop_ref as R  # noqa: E402
from tests._common import FULL, SMALL, load_golden, make_args, max_rel  # noqa: E402
from tests.test_gpu_dropout import case_inputs, check_against_reference, model_call, train_model  # noqa: E402
from worddiffusion_amd import Diffusion, UNetModel, UNetModelPhosc  # noqa: E402
from worddiffusion_amd.synthetic import fill_module_, synthetic_tensor  # noqa: E402

DEV = "cuda:0"
HW = (32, 64)
CLS = {"base": UNetModel, "phosc": UNetModelPhosc}


class IdentityVAE:
    def decode(self, z):
        return types.SimpleNamespace(sample=z)


def _model(cls, cfg, seed, **args_kw):
    return fill_module_(cls(args=make_args(device=DEV, **args_kw), **cfg), seed).to(DEV).eval()


def _same_bits(a, b):
    return torch.equal(a.cpu().contiguous().view(torch.int32), b.cpu().contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ 1. forwards
@pytest.mark.parametrize("tag", ["base", "phosc"])
def test_writer_keep_forward_matches_reference(golden_dir, tag):
    g = load_golden(golden_dir, "writer_free")
    m = _model(CLS[tag], SMALL, int(g[tag + "_seed"]))
    x, t, ctx, y = (torch.from_numpy(g[tag + "_" + k]).to(DEV) for k in ("x", "t", "context", "y"))
    B = x.shape[0]

    def fwd(**kw):
        with torch.no_grad():
            return m(x, None, timesteps=t, context=ctx, y=y, **kw).cpu()

    plain = fwd()
    free, cond = fwd(writer_keep=False), fwd(writer_keep=torch.ones(B, dtype=torch.bool))
    e_free, e_cond = max_rel(free, g[tag + "_out_free"]), max_rel(cond, g[tag + "_out_cond"])
    print(f"writer_keep forward {tag}: all dropped max_rel {e_free:.3e}, all kept {e_cond:.3e}; all kept == no argument bit for "
          f"bit: {_same_bits(cond, plain)}; all-False tensor == False: {_same_bits(fwd(writer_keep=torch.zeros(B, dtype=torch.uint8)), free)}")
    assert e_free < 1e-4 and e_cond < 1e-4
    assert max_rel(plain, g[tag + "_out_cond"]) < 1e-4 and max_rel(free, g[tag + "_out_cond"]) > 1e-3
    # a mixed mask: every sample agrees with the all-kept or the all-dropped forward of the same batch
    mask = torch.tensor([True, False, True])
    mixed = fwd(writer_keep=mask.to(DEV))
    errs = [max_rel(mixed[b], (cond if mask[b] else free)[b]) for b in range(B)]
    bit = all(_same_bits(mixed[b], (cond if mask[b] else free)[b]) for b in range(B))
    print(f"writer_keep forward {tag}: mixed mask against the uniform forwards, max_rel per sample {['%.2e' % e for e in errs]}, "
          f"bit-equal: {bit}")
    assert max(errs) < 1e-4
    assert fwd(writer_keep=mask.to(torch.uint8)).equal(mixed)  # uint8 on the host, bool on the device: one argument
    # the plan without the argument is untouched: same key set apart from the new plan's, same bits afterwards
    assert _same_bits(fwd(), plain)
    keys = list(m.engine._plans)
    assert sum(("writer_keep",) in k for k in keys) == 1 and sum(("writer_keep",) not in k for k in keys) == 1


def test_writer_keep_errors():
    m = _model(UNetModel, dict(SMALL, num_classes=339), 3, interpolation=True)
    x = torch.randn(2, 4, 4, 8, device=DEV)
    t = torch.tensor([3, 3], device=DEV)
    ctx = torch.full((2, 10), 52, dtype=torch.int64, device=DEV)
    y = torch.tensor([1, 2], device=DEV)
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="mix_rate"):
            m(x, None, timesteps=t, context=ctx, y=y, mix_rate=0.5, writer_keep=False)
        with pytest.raises(NotImplementedError, match="return_attention"):
            m(x, None, timesteps=t, context=ctx, y=y, return_attention=True, writer_keep=False)
        for bad in (torch.tensor([1.0, 0.0]), torch.tensor([True]), True):
            with pytest.raises(ValueError, match="writer_keep"):
                m(x, None, timesteps=t, context=ctx, y=y, writer_keep=bad)
        assert torch.isfinite(m(x, None, timesteps=t, context=ctx, y=y, writer_keep=False)).all()  # without mix_rate: no interpolation
        flag = _model(UNetModel, SMALL, 3, imgConditioned=1)
        with pytest.raises(NotImplementedError, match="writer_keep=False"):
            flag(x, None, timesteps=t, context=ctx, y=y)
        uncond = _model(UNetModel, dict(SMALL, num_classes=None), 3)
        with pytest.raises(ValueError, match="class-conditional"):
            uncond(x, None, timesteps=t, context=ctx, writer_keep=False)


# ------------------------------------------------------------------------------------------------ 2. autograd, mixed mask
def reference64_keep(variant, B, hw, seeds, keep):
    x, inp, eps = case_inputs(B, hw, seeds)
    sd = {k: torch.from_numpy(synthetic_tensor(k, s, seeds[0])).double().requires_grad_(True)
          for k, s in U.state_dict_shapes(FULL, variant)}
    orc = R.KeepOracle(FULL, sd, variant, False)
    orc.keep = keep
    pred = orc(x.double(), inp["t"], inp["context"], inp["y"], None)
    loss = torch.nn.functional.mse_loss(pred, eps.double())
    loss.backward()
    return pred.detach(), float(loss.detach()), {k: v.grad for k, v in sd.items() if v.grad is not None}


@pytest.mark.parametrize("variant,B,hw,keep", [("base", 3, (8, 16), [True, False, True]), ("phosc", 2, (8, 32), [False, True])])
def test_writer_keep_gradients_against_the_oracle(variant, B, hw, keep):
    seeds = (21, 300 + B, 4)
    x, inp, eps = case_inputs(B, hw, seeds)
    keep = np.array(keep)
    y = inp["y"]
    assert len(set(y.tolist())) == B  # distinct writers: the dropped sample's row is named by no kept sample
    m = train_model(variant, seeds[0], dropout=0)
    kw = dict(timesteps=inp["t"].to(DEV), context=inp["context"].to(DEV), y=y.to(DEV), writer_keep=torch.from_numpy(keep).to(DEV))
    pred = m(x.to(DEV), **kw) if variant == "base" else m(x.to(DEV), None, **kw)
    loss = torch.nn.MSELoss()(eps.to(DEV), pred)
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    check_against_reference(pred, float(loss.detach()), grads, reference64_keep(variant, B, hw, seeds, keep),
                            f"writer_keep {keep.astype(int).tolist()} FULL {variant} B={B} {hw}")
    lab = grads["label_emb.weight"].cpu()
    kept_rows = sorted(set(y[torch.from_numpy(keep)].tolist()))
    others = torch.ones(lab.shape[0], dtype=torch.bool)
    others[kept_rows] = False
    assert not bool(lab[others].view(torch.int32).any()), "a writer whose samples were all dropped got a gradient"
    assert all(bool(lab[r].any()) for r in kept_rows)
    plan = list(m.train_engine._tplans.values())[0]
    assert torch.equal(plan.writer_keep.cpu(), torch.from_numpy(keep).to(torch.uint8))
    assert sum(fn.__name__ == "wd_label_rows_keep" for fn, _, _ in plan.step) == 1
    # without the argument: the parent's plan, no such launch
    model_call(m, variant, x, inp).sum().backward()
    plan = list(m.train_engine._tplans.values())[0]
    assert not any(fn.__name__ == "wd_label_rows_keep" for fn, _, _ in plan.step) and plan.writer_keep is None


# ------------------------------------------------------------------------------------------------ 3. guided trajectories
@pytest.mark.parametrize("tag,variant", [("gb3", "base"), ("gb025", "base"), ("gp3", "phosc"), ("gp025", "phosc")])
def test_guided_trajectory_matches_reference(golden_dir, tag, variant):
    g = load_golden(golden_dir, "writer_free")
    T, s = int(g[tag + "_T"]), float(g[tag + "_cfg_scale"])
    n = g[tag + "_labels"].shape[0]
    args = make_args(device=DEV)
    m = _model(CLS[variant], SMALL, int(g[tag + "_seed"]))
    diff = Diffusion(noise_steps=T, img_size=HW, args=args)
    noise = torch.from_numpy(g[tag + "_noise"])
    labels = torch.from_numpy(g[tag + "_labels"])
    rec, preds = [], []
    img = diff.sampling(m, IdentityVAE(), n, str(g[tag + "_word"]), labels, args, cfg_scale=s, guidance="writer_free",
                        x_T=noise[0], noise=list(noise[1:]), record=rec, record_pred=preds)
    st = diff.last_stats
    assert st["forwards_per_step"] == 2 and st["guidance"] == "writer_free" and st["model_calls"] == 2 * (T - 1) == g[tag + "_pred"].shape[0]
    ref_pred = torch.from_numpy(g[tag + "_pred"])
    worst_single = worst_guided = 0.0
    for k, p in enumerate(preds):
        assert len(p) == 3
        for f in range(2):
            worst_single = max(worst_single, max_rel(p[f].cpu(), ref_pred[2 * k + f]))
        guided = torch.lerp(ref_pred[2 * k + 1], ref_pred[2 * k], s)  # train.py:228
        worst_guided = max(worst_guided, max_rel(p[2].cpu(), guided))
    xs = torch.stack([r.cpu() for r in rec])
    ex = max_rel(xs, g[tag + "_x_per_step"])
    eimg = float((img - torch.from_numpy(g[tag + "_image"])).abs().max())
    print(f"writer-free trajectory {tag}: single predictions max_rel {worst_single:.3e}, guided {worst_guided:.3e}, x {ex:.3e}, "
          f"image max abs {eimg:.3e}")
    assert worst_single < 1e-4
    assert worst_guided < (abs(s) + abs(1 - s)) * 1e-4
    assert xs.shape == tuple(g[tag + "_x_per_step"].shape) and ex < 1e-4
    assert eimg < 1e-3


def _keep_oracle64(variant, seed, phosc_on=False):
    sd = {k: torch.from_numpy(synthetic_tensor(k, s, seed)).double() for k, s in U.state_dict_shapes(SMALL, variant)}
    return R.KeepOracle(SMALL, sd, variant, phosc_on)


def _guided(orc, ctx, labels, ph, n, s):
    def model(x, t):
        orc.keep = np.ones(n, bool)
        cond = orc(x, t, ctx, labels, ph)
        orc.keep = np.zeros(n, bool)
        free = orc(x, t, ctx, labels, ph)
        return torch.lerp(free, cond, s)
    return model


@pytest.mark.parametrize("scale", [3.0, 0.25])
@pytest.mark.parametrize("which,variant", [("ddim", "base"), ("ddim", "phosc"), ("dpmpp", "base"), ("dpmpp", "phosc")])
def test_guided_ddim_and_dpmpp_match_their_host_specifications(which, variant, scale):
    T, S, n, seed = 8, 4, 3, 9
    phosc_on = variant == "phosc"
    args = make_args(device=DEV, phosc=1 if phosc_on else 0)
    m = _model(CLS[variant], SMALL, seed, phosc=1 if phosc_on else 0)
    diff = Diffusion(noise_steps=T, img_size=HW, args=args)
    g = torch.Generator().manual_seed(3)
    x_T = torch.randn(n, 4, 4, 8, generator=g)
    noise = [torch.randn(n, 4, 4, 8, generator=g) for _ in range(S)]
    labels = torch.tensor([1, 7, 10], dtype=torch.int64)
    word = "Moving"
    ph = torch.randint(0, 2, (n, 37), generator=g) if phosc_on else None
    ctx = torch.tensor([D.label_padding(word)] * n, dtype=torch.int64)
    ref_model = _guided(_keep_oracle64(variant, seed, phosc_on), ctx, labels, ph, n, scale)
    rec, ref_rec = [], []
    kw = dict(x_T=x_T, record=rec, phoscLabels=ph, cfg_scale=scale, guidance="writer_free")
    if which == "ddim":
        eta, tau = 0.7, [7, 5, 3, 1]
        out = diff.sampling_ddim(m, None, n, word, labels, args, steps=S, eta=eta, noise=noise, **kw)
        with torch.no_grad():
            ref = DDIM.sampling(ref_model, x_T, T, tau, eta, noise, record=ref_rec)
        bar = 1e-4
    else:
        tau = DPM.timesteps(T, S)
        out = diff.sampling_dpmpp(m, None, n, word, labels, args, steps=S, order=2, **kw)
        with torch.no_grad():
            ref = DPM.sampling(ref_model, x_T, T, tau, 2, record=ref_rec)
        bar = 1e-4 * (1 + 2 * float(DPM.tables(T, tau, 2)[4].max()))
    st = diff.last_stats
    assert (st["sampler"], st["timesteps"], st["forwards_per_step"], st["model_calls"], st["guidance"]) == \
        (which, tau, 2, 2 * S, "writer_free")
    xs = torch.stack([r.cpu() for r in rec] + [out.cpu()])
    ref_xs = torch.stack(ref_rec + [ref])
    assert xs.shape == ref_xs.shape == (S + 1, n, 4, 4, 8)
    errs = [max_rel(xs[k], ref_xs[k]) for k in range(S + 1)]
    print(f"guided {which} {variant} scale {scale}: bar {bar:.3e}, max_rel per state {['%.2e' % e for e in errs]}")
    assert max(errs) < bar
    del kw["record"]
    again = getattr(diff, "sampling_" + which)(m, None, n, word, labels, args, steps=S, **(dict(eta=0.7, noise=noise) if which == "ddim"
                                                                                          else dict(order=2)), **kw)
    assert diff.last_stats["graph"] and torch.equal(again, out)  # the graph replay gives the recorded eager run's bits


# ------------------------------------------------------------------------------------------------ 4. graph, no-op cases, plans
def test_guided_graph_replay_equals_eager_launches_across_table_chunks(monkeypatch):
    from worddiffusion_amd import engine
    monkeypatch.setattr(engine, "FILM_CHUNK_ROWS", 8)
    args = make_args(device=DEV)
    m = _model(UNetModelPhosc, SMALL, 9)
    diff = Diffusion(noise_steps=12, img_size=HW, args=args)
    labels = torch.tensor([4, 5, 6], dtype=torch.int64)
    outs = []
    for use_graph in (True, False):
        outs.append(diff.sampling(m, None, 3, "text", labels, args, use_graph=use_graph, seed=21, guidance="writer_free"))
        assert diff.last_stats["graph"] == use_graph and diff.last_stats["forwards_per_step"] == 2
    (P,) = m.engine._plans.values()
    assert P.film_nchunks == 2 and P.guide == 2 and P.mix == 0
    assert torch.equal(outs[0], outs[1])
    assert torch.isfinite(outs[0]).all() and float(outs[0].std()) > 0
    # the writer and the scale matter
    assert not torch.equal(diff.sampling(m, None, 3, "text", labels + 1, args, seed=21, guidance="writer_free"), outs[0])
    assert not torch.equal(diff.sampling(m, None, 3, "text", labels, args, seed=21, guidance="writer_free", cfg_scale=1.5), outs[0])


def test_plain_calls_are_untouched_and_scale_zero_is_the_plain_call():
    args = make_args(device=DEV)
    m = _model(UNetModel, SMALL, 5)
    diff = Diffusion(noise_steps=9, img_size=HW, args=args)
    labels = torch.tensor([1, 2, 3], dtype=torch.int64)
    kw = dict(n=3, x_text="MOVE", labels=labels, args=args, seed=11)
    before = diff.sampling(m, None, **kw)
    assert diff.last_stats["forwards_per_step"] == 1 and "guidance" not in diff.last_stats
    (key0,) = m.engine._plans
    nstep0 = len(m.engine._plans[key0].step)
    assert torch.equal(diff.sampling(m, None, cfg_scale=7, **kw), before)  # cfg_scale stays inert without the argument
    zero = diff.sampling(m, None, guidance="writer_free", cfg_scale=0, **kw)  # train.py:223: one forward
    assert torch.equal(zero, before) and diff.last_stats["forwards_per_step"] == 1 and "guidance" not in diff.last_stats
    assert list(m.engine._plans) == [key0]
    guided = diff.sampling(m, None, guidance="writer_free", **kw)
    assert diff.last_stats["forwards_per_step"] == 2 and not torch.equal(guided, before)
    assert set(m.engine._plans) == {key0, key0 + (("guide", 2),)}
    after = diff.sampling(m, None, **kw)
    assert torch.equal(after, before) and len(m.engine._plans[key0].step) == nstep0
    for which, extra in (("sampling_ddim", dict(steps=4)), ("sampling_dpmpp", dict(steps=4))):
        fn = getattr(diff, which)
        plain = fn(m, None, **kw, **extra)
        assert torch.equal(fn(m, None, guidance="writer_free", cfg_scale=0, **kw, **extra), plain)
        assert not torch.equal(fn(m, None, guidance="writer_free", **kw, **extra), plain)
        assert torch.equal(fn(m, None, **kw, **extra), plain)
    # scale 1: lerp(free, cond, 1) is cond itself - the plain trajectory from two forwards - and the maps, read from the
    # conditional forward alone, are the plain call's
    one = diff.sampling(m, None, guidance="writer_free", cfg_scale=1, attention=True, **kw)
    maps = {k: v.clone() for k, v in diff.last_attention.items()}
    assert diff.last_stats["forwards_per_step"] == 2
    ref = diff.sampling(m, None, attention=True, **kw)
    assert torch.equal(one, ref)
    for k, v in diff.last_attention.items():
        assert torch.equal(maps[k], v), k


def test_guided_step_has_the_launches_of_the_two_forward_interpolation_step():
    """The captured guided step runs what the two-forward step of the reference's interpolation mode runs (``plan`` mix = 2):
    that plan predates this one, so the number comes from there."""
    import random
    cfg = dict(SMALL, num_classes=339)
    labels = torch.tensor([4, 5, 6], dtype=torch.int64)
    counts = {}
    for mode in ("mix", "guide"):
        inter = mode == "mix"
        args = make_args(device=DEV, interpolation=inter)
        m = _model(UNetModelPhosc, cfg, 9, interpolation=inter)
        diff = Diffusion(noise_steps=6, img_size=HW, args=args)
        random.seed(31)
        diff.sampling(m, None, 3, "text", labels, args, seed=21, **(dict(mix_rate=0.37) if inter else dict(guidance="writer_free")))
        assert diff.last_stats["forwards_per_step"] == 2
        (P,) = m.engine._plans.values()
        assert (P.mix, P.guide) == ((2, 0) if inter else (0, 2))
        counts[mode] = (len(P.step), len(P.step1), [fn.__name__ for fn, _, _ in P.step + P.step1])
    assert counts["guide"] == counts["mix"]
    with pytest.raises(NotImplementedError):
        m.engine.plan(3, 4, 8, 10, 0, film_steps=6, mix=2, guide=2)


def test_guidance_composes_with_known_regions_offsets_and_the_phosc_entry_point():
    args = make_args(device=DEV, phosc=1)
    m = _model(UNetModelPhosc, SMALL, 6, phosc=1)
    diff = Diffusion(noise_steps=9, img_size=HW, args=args)
    n = 3
    labels = torch.tensor([1, 2, 3], dtype=torch.int64)
    g = torch.Generator().manual_seed(1)
    ph = torch.randint(0, 2, (n, 37), generator=g)
    known = torch.randn(n, 4, 4, 8, generator=g) * 0.8
    kw = dict(seed=11, guidance="writer_free")
    # an all-ones mask: the trajectory ends on the known latents themselves, as the plain known call's does
    ones = torch.ones(4, 8)
    plain = diff.sampling_phosc(m, None, n, "MOVE", ph, labels, args, seed=11, known=known, known_mask=ones)
    full = diff.sampling_phosc(m, None, n, "MOVE", ph, labels, args, known=known, known_mask=ones, **kw)
    assert diff.last_stats["known"] and diff.last_stats["forwards_per_step"] == 2
    assert _same_bits(full, plain) and _same_bits(full, known)
    # a column mask: the kept columns are the known latents, the rest is guided
    cols = torch.zeros(4, 8)
    cols[:, :4] = 1
    part = diff.sampling_phosc(m, None, n, "MOVE", ph, labels, args, known=known, known_mask=cols, **kw)
    unguided = diff.sampling_phosc(m, None, n, "MOVE", ph, labels, args, seed=11, known=known, known_mask=cols)
    assert _same_bits(part[..., :4], known[..., :4]) and not torch.equal(part[..., 4:], unguided[..., 4:])
    # start: from the noised known latents
    started = diff.sampling_phosc(m, None, n, "MOVE", ph, labels, args, known=known, start=5, **kw)
    assert diff.last_stats["start"] == 5 and diff.last_stats["steps"] == 5 and torch.isfinite(started).all()
    # rows 1..2 of the batch at their global offset (another batch size may tile its GEMMs differently: the forward's bar)
    whole = diff.sampling_phosc(m, None, n, "MOVE", ph, labels, args, **kw)
    tail = diff.sampling_phosc(m, None, 2, "MOVE", ph[1:], labels[1:], args, sample_offset=1, **kw)
    err = max_rel(tail.cpu(), whole[1:].cpu())
    print(f"guided rows 1..2 of n = 3 against n = 2 at sample_offset 1: max_rel {err:.3e}")
    assert err < 1e-4
    # refused together with the interpolation modes, on the host
    diff.last_stats = {}
    with pytest.raises(ValueError, match="interpolation"):
        diff.sampling_phosc(m, None, n, "MOVE", ph, labels, args, mix_rate=0.5, style_pairs=(1, 2), **kw)
    with pytest.raises(ValueError, match="guidance"):
        diff.sampling_phosc(m, None, n, "MOVE", ph, labels, args, seed=11, guidance="text_free")
    assert diff.last_stats == {}


def test_eval_loss_scores_the_writer_free_branch():
    args = make_args(device=DEV)
    m = _model(UNetModel, SMALL, 5)
    diff = Diffusion(noise_steps=9, img_size=HW, args=args)
    g = torch.Generator().manual_seed(2)
    lat = torch.randn(3, 4, 4, 8, generator=g).to(DEV)
    ctx = torch.full((3, 10), 52, dtype=torch.int64)
    y = torch.tensor([1, 2, 3])
    t = torch.tensor([2, 5, 8])
    plain = diff.eval_loss(m, lat, ctx, y, t, seed=3)
    kept = diff.eval_loss(m, lat, ctx, y, t, seed=3, writer_keep=torch.ones(3, dtype=torch.bool))
    free = diff.eval_loss(m, lat, ctx, y, t, seed=3, writer_keep=False)
    mixed = diff.eval_loss(m, lat, ctx, y, t, seed=3, writer_keep=torch.tensor([True, False, True]))
    assert plain.shape == free.shape == (3,) and max_rel(kept.cpu(), plain.cpu()) < 1e-4
    assert not torch.equal(free, plain)
    assert max_rel(mixed.cpu(), torch.stack([plain[0], free[1], plain[2]]).cpu()) < 1e-4
