"""Writer-style interpolation (``mix_rate``) on the GPU: the three kernels against float64, the model forwards and the guided
sampling loop against what the reference's own modules computed (``tests/golden/interp.npz``, ``tools/make_golden_interp.py``),
graph replay against eager launches, the fixed-pair mode's properties, the errors and the driver.

Bars: 1e-4 max-norm relative for a forward and for the states of a short trajectory (the project's split-bf16 bar,
``tests/test_gpu_samplers.py``); (|s| + |1 - s|) 1e-4 for the guided prediction ``first - (first - second) (1 - s)``, whose two
terms carry the two forwards' errors scaled by |s| and |1 - s|."""
import os
import random
import struct
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests._common import FULL, SMALL, load_golden, make_args, max_rel  # noqa: E402
from worddiffusion_amd import Diffusion, UNetModel, UNetModelPhosc  # noqa: E402
from worddiffusion_amd import _native as N  # noqa: E402
from worddiffusion_amd.diffusion import draw_style_pairs  # noqa: E402
from worddiffusion_amd.synthetic import fill_module_  # noqa: E402

DEV = "cuda:0"
CFG = dict(SMALL, num_classes=339)


class IdentityVAE:
    def decode(self, z):
        return types.SimpleNamespace(sample=z)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _model(cls, cfg, seed, **args_kw):
    return fill_module_(cls(args=make_args(device=DEV, **args_kw), **cfg), seed).to(DEV).eval()


# ------------------------------------------------------------------------------------------------ 1. the no-op case
def test_mix_rate_is_ignored_without_args_interpolation():
    """full_sampling.py:171 passes mix_rate on its default branch; a model built with interpolation=False ignores it
    (unet.py:1558): every call form gives the bits of the call without it and Python's ``random`` is not consumed."""
    args = make_args(device=DEV)
    m = _model(UNetModelPhosc, SMALL, 5)
    diff = Diffusion(noise_steps=9, img_size=(32, 64), args=args)
    labels = torch.tensor([1, 2, 3], dtype=torch.int64)
    w = "MOVE"
    random.seed(77)
    state = random.getstate()
    vae = IdentityVAE()
    plain = diff.sampling(m, vae, n=len(labels), x_text=w, labels=labels, args=args, seed=11)
    assert torch.equal(diff.sampling(m, vae, n=len(labels), x_text=w, labels=labels, args=args, mix_rate=0.37, seed=11), plain)
    assert torch.equal(diff.sample(m, vae, n=len(labels), x_text=w, labels=labels, args=args, mix_rate=0.37, seed=11), plain)
    s3 = diff.sampling3(0, None, [w] * 3, None, m, m, None, 0, 1, 3, w, labels, args, seed=11)
    assert torch.equal(diff.sampling3(0, None, [w] * 3, None, m, m, None, 0, 1, 3, w, labels, args, mix_rate=0.37, seed=11), s3)
    pargs = make_args(device=DEV, phosc=1)
    mp = _model(UNetModelPhosc, SMALL, 6, phosc=1)
    ph = torch.randint(0, 2, (3, 37), generator=torch.Generator().manual_seed(1))
    pp = diff.sampling_phosc(mp, vae, 3, w, ph, labels, pargs, seed=11)
    assert torch.equal(diff.sampling_phosc(mp, vae, 3, w, ph, labels, pargs, mix_rate=0.37, seed=11), pp)
    assert random.getstate() == state
    assert torch.isfinite(plain).all() and float(plain.std()) > 0


# ------------------------------------------------------------------------------------------------ 2. kernels
def _planes_value(pl):
    return pl[0].float().double() + pl[1].float().double()


def test_emb_combine_mix_kernel():
    lib = N.lib()
    T, B, ted, ncls = 19, 5, 256, 339  # ragged batch; 19 timesteps = two chunks of 10 and 9 rows of ``time`` in the second call
    g = torch.Generator().manual_seed(3)
    time = torch.randn(T, ted, generator=g)
    label = torch.randn(ncls, ted, generator=g)
    pairs = torch.randint(0, ncls, (T, B, 2), generator=g, dtype=torch.int32)
    m = torch.rand(B, generator=g)
    m[0], m[1] = 0.0, 1.0
    td, ld, pd, md = (t.to(DEV) for t in (time, label, pairs, m))
    out = torch.zeros(2, T * B, ted, dtype=torch.bfloat16, device=DEV)
    for t0, nt in ((0, 10), (10, 9)):  # chunk by chunk, as the engine calls it
        N.check(lib.wd_emb_combine_mix(td[t0].data_ptr(), ld.data_ptr(), pd[t0].data_ptr(), md.data_ptr(), ncls, nt, B, ted,
                                       out[0, t0 * B].data_ptr(), out[1, t0 * B].data_ptr(), ted, _st()), "wd_emb_combine_mix")
    torch.cuda.synchronize()
    l1 = label.double()[pairs[..., 0].long()]
    l2 = label.double()[pairs[..., 1].long()]
    md64 = m.double()[None, :, None]
    ref = torch.nn.functional.silu(time.double()[:, None, :] + ((1 - md64) * l1 + md64 * l2)).reshape(T * B, ted)
    got = _planes_value(out.cpu())
    # hi = bf16(v), lo = bf16(v - hi): two roundings of relative 2^-9 each leave 2^-18 |v|; the fp32 sums and SiLU a few 2^-24
    err = (got - ref).abs()
    print(f"wd_emb_combine_mix: max |err| / (|v| + 1) = {float((err / (ref.abs() + 1)).max()):.3e}")
    assert (err <= 2.0 ** -16 * ref.abs() + 1e-6).all()
    # m = 0 / m = 1 with one pair for every t: the planes of wd_emb_combine for y = s1 / y = s2, bit for bit
    fixed = torch.randint(0, ncls, (B, 2), generator=g, dtype=torch.int32)
    pf = fixed[None].expand(T, B, 2).contiguous().to(DEV)
    for mv, col in ((0.0, 0), (1.0, 1)):
        mm = torch.full((B,), mv, device=DEV)
        a = torch.zeros(2, T * B, ted, dtype=torch.bfloat16, device=DEV)
        b = torch.zeros_like(a)
        N.check(lib.wd_emb_combine_mix(td.data_ptr(), ld.data_ptr(), pf.data_ptr(), mm.data_ptr(), ncls, T, B, ted, a[0].data_ptr(),
                                       a[1].data_ptr(), ted, _st()), "wd_emb_combine_mix")
        y = fixed[:, col].long().to(DEV)
        N.check(lib.wd_emb_combine(td.data_ptr(), ld.data_ptr(), y.data_ptr(), ncls, T, B, ted, b[0].data_ptr(), b[1].data_ptr(), ted,
                                   _st()), "wd_emb_combine")
        torch.cuda.synchronize()
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), mv
    # ids outside the table are clamped, never read
    bad = torch.tensor([[-5, 10 ** 6]] * B, dtype=torch.int32)[None].expand(T, B, 2).contiguous().to(DEV)
    mm = torch.zeros(B, device=DEV)
    a = torch.zeros(2, T * B, ted, dtype=torch.bfloat16, device=DEV)
    N.check(lib.wd_emb_combine_mix(td.data_ptr(), ld.data_ptr(), bad.data_ptr(), mm.data_ptr(), ncls, T, B, ted, a[0].data_ptr(),
                                   a[1].data_ptr(), ted, _st()), "wd_emb_combine_mix")
    torch.cuda.synchronize()
    ref0 = torch.nn.functional.silu(time.double() + label.double()[0])[:, None, :].expand(T, B, ted).reshape(T * B, ted)
    assert ((_planes_value(a.cpu()) - ref0).abs() <= 2.0 ** -16 * ref0.abs() + 1e-6).all()
    assert lib.wd_emb_combine_mix(td.data_ptr(), ld.data_ptr(), None, md.data_ptr(), ncls, T, B, ted, a[0].data_ptr(), None, ted,
                                  _st()) == N.WD_EINVAL


def test_label_mix_kernel():
    lib = N.lib()
    B, ted, ncls = 7, 1280, 339
    g = torch.Generator().manual_seed(4)
    label = torch.randn(ncls, ted, generator=g)
    pairs = torch.randint(0, ncls, (B, 2), generator=g, dtype=torch.int32)
    m = torch.rand(B, generator=g)
    m[0], m[1] = 0.0, 1.0
    out = torch.zeros(B, ted, device=DEV)
    ld, pd, md = label.to(DEV), pairs.to(DEV), m.to(DEV)
    N.check(lib.wd_label_mix(ld.data_ptr(), pd.data_ptr(), md.data_ptr(), ncls, B, ted, out.data_ptr(), _st()), "wd_label_mix")
    torch.cuda.synchronize()
    l1, l2 = label[pairs[:, 0].long()], label[pairs[:, 1].long()]
    md64 = m.double()[:, None]
    ref = (1 - md64) * l1.double() + md64 * l2.double()
    got = out.cpu()
    # 1 - m, two products and a sum in fp32: four roundings of 2^-24 on terms no larger than max(|l1|, |l2|)
    bound = 4 * 2.0 ** -24 * torch.maximum(l1.abs(), l2.abs()).double() + 1e-30
    print(f"wd_label_mix: max |err| / bound = {float(((got.double() - ref).abs() / bound).max()):.3f}")
    assert ((got.double() - ref).abs() <= bound).all()
    assert torch.equal(got[0], l1[0]) and torch.equal(got[1], l2[1])


@pytest.mark.parametrize("scale", [3.0, 0.25])
@pytest.mark.parametrize("given_noise", [False, True])
def test_ddpm_step_cfg_kernel(scale, given_noise):
    lib = N.lib()
    B, n = 5, 1024
    g = torch.Generator().manual_seed(6)
    x, first, second, z = (torch.randn(B, n, generator=g) for _ in range(4))
    Tn = 50
    ca, cb, cs = (torch.rand(Tn, generator=g) + 0.5 for _ in range(3))
    cad, cbd, csd = ca.to(DEV), cb.to(DEV), cs.to(DEV)
    fd, sd, zd = first.to(DEV), second.to(DEV), z.to(DEV)
    for t in (17, 1):  # t = 1: no noise term
        t_dev = torch.tensor([t], dtype=torch.int32, device=DEV)
        xa, xb = x.to(DEV), x.to(DEV)
        eps = torch.zeros(B, n, device=DEV)
        noise = zd.data_ptr() if given_noise else None
        N.check(lib.wd_ddpm_step_cfg(xa.data_ptr(), fd.data_ptr(), sd.data_ptr(), scale, eps.data_ptr(), B, n, cad.data_ptr(),
                                     cbd.data_ptr(), csd.data_ptr(), t_dev.data_ptr(), noise, 123, 40, _st()), "wd_ddpm_step_cfg")
        N.check(lib.wd_ddpm_step(xb.data_ptr(), eps.data_ptr(), B, n, cad.data_ptr(), cbd.data_ptr(), csd.data_ptr(),
                                 t_dev.data_ptr(), noise, 123, 40, _st()), "wd_ddpm_step")
        torch.cuda.synchronize()
        # the update half: wd_ddpm_step fed the combined prediction, bit for bit (same Philox stream)
        assert torch.equal(xa, xb)
        assert not torch.equal(xa.cpu(), x)
        f64, s64 = first.double(), second.double()
        ref = f64 - (f64 - s64) * (1 - scale) if abs(scale) >= 0.5 else s64 + scale * (f64 - s64)
        # three fp32 roundings on terms bounded by (1 + |s| + |1 - s|) max(|first|, |second|)
        bound = 4 * 2.0 ** -24 * (1 + abs(scale) + abs(1 - scale)) * torch.maximum(first.abs(), second.abs()).double()
        assert ((eps.cpu().double() - ref).abs() <= bound).all()
        if scale == 3.0:  # the form torch.lerp takes for a weight >= 0.5
            assert torch.equal(eps.cpu(), torch.lerp(second, first, scale))
        # eps_out is optional
        xc = x.to(DEV)
        N.check(lib.wd_ddpm_step_cfg(xc.data_ptr(), fd.data_ptr(), sd.data_ptr(), scale, None, B, n, cad.data_ptr(),
                                     cbd.data_ptr(), csd.data_ptr(), t_dev.data_ptr(), noise, 123, 40, _st()), "wd_ddpm_step_cfg")
        torch.cuda.synchronize()
        assert torch.equal(xc, xa)


# ------------------------------------------------------------------------------------------------ 3. forward goldens
@pytest.mark.parametrize("tag,cls", [("base", UNetModel), ("phosc", UNetModelPhosc)])
def test_interpolation_forward_matches_reference(golden_dir, tag, cls):
    g = load_golden(golden_dir, "interp")
    m = _model(cls, CFG, int(g[tag + "_seed"]), interpolation=True)
    x, t, ctx, y = (torch.from_numpy(g[tag + "_" + k]).to(DEV) for k in ("x", "t", "context", "y"))
    random.seed(int(g[tag + "_rseed"]))
    with torch.no_grad():
        out = m(x, None, timesteps=t, context=ctx, y=y, mix_rate=float(g["mix_rate"]))
    state = random.getstate()
    random.seed(int(g[tag + "_rseed"]))
    assert draw_style_pairs(1) == [tuple(int(v) for v in g[tag + "_pair"])] and random.getstate() == state
    err = max_rel(out.cpu(), g[tag + "_out"])
    print(f"interp forward {tag}: max_rel {err:.3e}")
    assert err < 1e-4
    # without mix_rate the same model takes the writer ids (unet.py:1575) - a different result
    with torch.no_grad():
        plain = m(x, None, timesteps=t, context=ctx, y=y)
    assert max_rel(plain.cpu(), g[tag + "_out"]) > 1e-3


# ------------------------------------------------------------------------------------------------ 4. trajectories
@pytest.mark.parametrize("tag,fps", [("cfg3", 2), ("cfg0", 1)])
def test_guided_interpolation_trajectory_matches_reference(golden_dir, tag, fps):
    g = load_golden(golden_dir, "interp")
    T, s = int(g[tag + "_T"]), float(g[tag + "_cfg_scale"])
    n = g[tag + "_labels"].shape[0]
    args = make_args(device=DEV, interpolation=True)
    m = _model(UNetModelPhosc, CFG, int(g[tag + "_seed"]), interpolation=True)
    diff = Diffusion(noise_steps=T, img_size=(32, 64), args=args)
    noise = torch.from_numpy(g[tag + "_noise"])
    labels = torch.from_numpy(g[tag + "_labels"])
    rec, preds = [], []
    random.seed(int(g[tag + "_rseed"]))
    img = diff.sampling(m, IdentityVAE(), n, str(g[tag + "_word"]), labels, args, mix_rate=float(g["mix_rate"]), cfg_scale=s,
                        x_T=noise[0], noise=list(noise[1:]), record=rec, record_pred=preds)
    state = random.getstate()
    random.seed(int(g[tag + "_rseed"]))
    assert draw_style_pairs(fps * (T - 1)) == [tuple(int(v) for v in p) for p in g[tag + "_pairs"]]
    assert random.getstate() == state  # the generator is where the reference's loop leaves it
    assert diff.last_stats["forwards_per_step"] == fps and diff.last_stats["model_calls"] == fps * (T - 1) == g[tag + "_pred"].shape[0]
    ref_pred = torch.from_numpy(g[tag + "_pred"])
    worst_single = worst_guided = 0.0
    for k, p in enumerate(preds):
        for f in range(fps):
            worst_single = max(worst_single, max_rel(p[f].cpu(), ref_pred[fps * k + f]))
        if fps == 2:
            guided = torch.lerp(ref_pred[2 * k + 1], ref_pred[2 * k], s)  # train.py:228
            worst_guided = max(worst_guided, max_rel(p[2].cpu(), guided))
    xs = torch.stack([r.cpu() for r in rec])
    ex = max_rel(xs, g[tag + "_x_per_step"])
    eimg = float((img - torch.from_numpy(g[tag + "_image"])).abs().max())
    print(f"interp trajectory {tag}: single predictions max_rel {worst_single:.3e}, guided {worst_guided:.3e}, x {ex:.3e}, "
          f"image max abs {eimg:.3e}")
    assert worst_single < 1e-4
    assert worst_guided < (abs(s) + abs(1 - s)) * 1e-4
    assert xs.shape == tuple(g[tag + "_x_per_step"].shape) and ex < 1e-4
    assert eimg < 1e-3


# ------------------------------------------------------------------------------------------------ 5. graph == eager
@pytest.mark.parametrize("mode", ["reference", "reference_cfg0", "fixed"])
def test_interpolation_graph_replay_equals_eager_launches(monkeypatch, mode):
    """... with the FiLM table cut into chunks of 8 timesteps, so that the 12-step schedule crosses a chunk boundary."""
    from worddiffusion_amd import engine
    monkeypatch.setattr(engine, "FILM_CHUNK_ROWS", 8)
    args = make_args(device=DEV, interpolation=mode != "fixed")
    m = _model(UNetModelPhosc, CFG, 9, interpolation=mode != "fixed")
    diff = Diffusion(noise_steps=12, img_size=(32, 64), args=args)
    labels = torch.tensor([4, 5, 6], dtype=torch.int64)
    kw = dict(mix_rate=0.37, seed=21)
    if mode == "fixed":
        kw.update(mix_rate=torch.tensor([0.0, 0.5, 1.0]), style_pairs=torch.tensor([[3, 7], [100, 2], [338, 0]]))
    if mode == "reference_cfg0":
        kw.update(cfg_scale=0)
    outs = []
    for use_graph in (True, False):
        random.seed(31)
        outs.append(diff.sampling(m, None, 3, "text", labels, args, use_graph=use_graph, **kw))
        assert diff.last_stats["graph"] == use_graph
        assert diff.last_stats["forwards_per_step"] == (2 if mode == "reference" else 1)
    P = next(iter(m.engine._plans.values()))
    assert P.film_nchunks == 2 and P.mix == (2 if mode == "reference" else 1)
    assert torch.equal(outs[0], outs[1])
    assert torch.isfinite(outs[0]).all() and float(outs[0].std()) > 0
    # the writers matter: other pairs, another result
    random.seed(32)
    if mode == "fixed":
        kw.update(style_pairs=(5, 6))
    assert not torch.equal(diff.sampling(m, None, 3, "text", labels, args, **kw), outs[0])


def test_sampling3_step_skipping_draws_one_pair_per_model_call(monkeypatch):
    """``sampling3`` on a model built with args.interpolation, same shapes: the skipped steps run the update alone (the second
    captured graph), call no model and draw no pair."""
    from worddiffusion_amd import engine
    monkeypatch.setattr(engine, "FILM_CHUNK_ROWS", 8)
    T = 12
    args = make_args(device=DEV, interpolation=True, fullSampling=False)
    m = _model(UNetModelPhosc, CFG, 9, interpolation=True)
    diff = Diffusion(noise_steps=T, img_size=(32, 64), args=args)
    labels = torch.tensor([4, 5, 6], dtype=torch.int64)
    calls = [i for i in reversed(range(1, T)) if Diffusion.sampling3_calls_model(i, T, 0)]
    assert calls == [11, 10, 5]

    def run(mix_rate, use_graph=True):
        random.seed(31)
        out = diff.sampling3(0, None, ["text"] * 3, None, m, m, None, 0, 1, 3, "text", labels, args, mix_rate=mix_rate,
                             seed=21, use_graph=use_graph)
        assert diff.last_stats["graph"] == use_graph
        assert diff.last_stats["model_calls"] == len(calls) and diff.last_stats["forwards_per_step"] == 1
        return out, random.getstate()

    (graph, after), (eager, after_eager) = run(0.37), run(0.37, use_graph=False)
    assert torch.equal(graph, eager)
    assert torch.isfinite(graph).all() and float(graph.std()) > 0
    random.seed(31)
    draw_style_pairs(len(calls))
    assert after == after_eager == random.getstate()
    assert not torch.equal(run(0.9)[0], graph)


# ------------------------------------------------------------------------------------------------ 6. fixed pairs
def test_fixed_pair_strip_properties_full_config():
    """B = 11 mix rates from 0 to 1 between two chosen writers, one word, on the FULL base config (interpolation not set)."""
    args = make_args(device=DEV)
    m = _model(UNetModel, FULL, 13)
    diff = Diffusion(noise_steps=6, img_size=(64, 256), args=args)
    s1, s2, B = 17, 301, 11
    unused = torch.zeros(B, dtype=torch.int64)
    random.seed(1)
    state = random.getstate()
    strip = diff.sampling(m, None, B, "getting", unused, args, mix_rate=torch.linspace(0, 1, B), style_pairs=(s1, s2), seed=44)
    assert diff.last_stats["forwards_per_step"] == 1 and diff.last_stats["model_calls"] == 5 and diff.last_stats["graph"]
    assert random.getstate() == state
    mix_ops = len(next(iter(m.engine._plans.values())).step)
    a = diff.sampling(m, None, B, "getting", torch.full((B,), s1), args, seed=44)
    plain_ops = [len(P.step) for P in m.engine._plans.values() if not P.mix]
    assert plain_ops == [mix_ops]  # the captured step of the fixed-pair mode has the launches of plain sampling, no more
    b = diff.sampling(m, None, B, "getting", torch.full((B,), s2), args, seed=44)
    assert torch.equal(strip[0], a[0])    # m = 0: writer s1, global sample 0
    assert torch.equal(strip[10], b[10])  # m = 1: writer s2, global sample 10
    assert not torch.equal(strip[0], strip[10]) and not torch.equal(a, b)
    # per-sample independence: sample 5 alone, at its global index.  (A batch of 1 may take other GEMM tilings than a batch
    # of 11, i.e. another fp32 summation order: held to the bar of one forward, not to bit equality.)
    one = diff.sampling(m, None, 1, "getting", unused[:1], args, mix_rate=torch.linspace(0, 1, B)[5:6], style_pairs=(s1, s2), seed=44,
                        sample_offset=5)
    err = max_rel(one[0].cpu(), strip[5].cpu())
    print(f"fixed pair: sample 5 of 11 against a batch of 1 at sample_offset 5: max_rel {err:.3e}")
    assert err < 1e-4
    assert max_rel(strip[4].cpu(), strip[5].cpu()) > 1e-3
    # [B, 2] pairs: each sample its own writers
    per = diff.sampling(m, None, B, "getting", unused, args, mix_rate=0.0, style_pairs=torch.tensor([[s1, s2]] * 10 + [[s2, s1]]),
                        seed=44)
    assert torch.equal(per[0], a[0]) and torch.equal(per[10], b[10])


# ------------------------------------------------------------------------------------------------ 7. errors
def test_interpolation_errors():
    args = make_args(device=DEV, interpolation=True)
    labels = torch.tensor([1, 2], dtype=torch.int64)
    small = _model(UNetModelPhosc, SMALL, 3, interpolation=True)  # 11 writers: nearly every draw from 0..338 is out of range
    diff = Diffusion(noise_steps=6, img_size=(32, 64), args=args)
    for bad in ((3, 11), (-1, 2), torch.tensor([[0, 1], [2, 400]])):
        with pytest.raises((IndexError, ValueError)):
            diff.sampling(small, None, 2, "a", labels, args, mix_rate=0.5, style_pairs=bad)
        assert diff.last_stats == {}  # refused on the host, before any launch
    with pytest.raises(ValueError):
        diff.sampling(small, None, 2, "a", labels, args, style_pairs=(1, 2))  # no mix_rate
    with pytest.raises(ValueError):
        diff.sampling(small, None, 2, "a", labels, args, mix_rate=0.5, style_pairs=(1, 2, 3))
    random.seed(int(1003))  # first pair (254, 286)
    with pytest.raises(IndexError):
        diff.sampling(small, None, 2, "a", labels, args, mix_rate=0.5)
    assert diff.last_stats == {}
    x = torch.randn(2, 4, 4, 8, device=DEV)
    t = torch.tensor([3, 3], device=DEV)
    ctx = torch.full((2, 10), 52, dtype=torch.int64, device=DEV)
    random.seed(1003)
    with torch.no_grad(), pytest.raises(IndexError):
        small(x, None, timesteps=t, context=ctx, y=labels.to(DEV), mix_rate=0.5)
    # in-range pairs run on the same model
    ok = diff.sampling(small, None, 2, "a", labels, args, mix_rate=0.5, style_pairs=(3, 10))
    assert torch.isfinite(ok).all()
    # autograd: the training forward does not interpolate
    big = _model(UNetModelPhosc, CFG, 3, interpolation=True).train()
    with pytest.raises(NotImplementedError):
        big(x, None, timesteps=t, context=ctx, y=labels.to(DEV), mix_rate=0.5)
    with torch.no_grad():
        assert torch.isfinite(big(x, None, timesteps=t, context=ctx, y=labels.to(DEV), mix_rate=0.5)).all()


# ------------------------------------------------------------------------------------------------ 8. driver
def test_driver_writes_one_strip_per_row(golden_dir, tmp_path, monkeypatch):
    from worddiffusion_amd import driver
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    lines = [ln for ln in open(os.path.join(golden_dir, "gt_samples.txt")).read().splitlines() if ln.strip()]
    rows_txt = [ln for ln in lines if not ln.startswith("#")][:2]
    gt = tmp_path / "gt.txt"
    gt.write_text("\n".join(rows_txt) + "\n")
    rows = driver.read_gt(str(gt))
    assert len(rows) == 2
    out = tmp_path / "out"
    driver.main(["--gt_train", str(gt), "--save_path", str(out), "--writer_dict", str(tmp_path / "writers.json"), "--emb_dim", "64",
                 "--num_heads", "2", "--noise_steps", "6", "--seed", "5", "--style_pair", "3", "7", "--mix_steps", "5"])
    for _, image, _ in rows:
        png = (out / "images" / f"{image}_interp.png").read_bytes()
        assert png[:8] == b"\x89PNG\r\n\x1a\n" and png[12:16] == b"IHDR"
        w, h = struct.unpack(">II", png[16:24])
        assert (w, h) == (5 * 32, 4 * 8)  # latents (no VAE given): 5 samples side by side, the 4 channels of 8 x 32 stacked
        lat = np.load(out / "images" / f"{image}_interp.npy")
        assert lat.shape == (5, 4, 8, 32) and np.isfinite(lat).all()
    # with a VAE the strip is the decoded images side by side
    args = make_args(device=DEV)
    m = _model(UNetModel, dict(SMALL, image_size=(64, 256), num_classes=339), 8)

    class UpVAE:  # stands in for a decoder: [N, 4, h, w] latents -> [N, 3, 8h, 8w]
        def decode(self, z):
            return types.SimpleNamespace(sample=torch.nn.functional.interpolate(z[:, :3], scale_factor=8).tanh())

    diff = Diffusion(noise_steps=6, img_size=(64, 256), args=args)
    start, strips = driver.interpolate(m, diff, rows[:1], args, (3, 7), 4, vae=UpVAE(), out_dir=str(out / "v"), seed=5, rank=0, world=1)
    assert start == 0 and strips[0].shape == (4, 3, 64, 256)
    png = (out / "v" / f"{rows[0][1]}_interp.png").read_bytes()
    assert struct.unpack(">II", png[16:24]) == (4 * 256, 64)
