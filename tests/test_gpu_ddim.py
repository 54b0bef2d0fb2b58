"""The DDIM sampler on the GPU: ``wd_ddim_step`` / ``wd_next_timestep`` against the same expression in unfused torch fp32 (bit
for bit) and against ``wd_ddpm_step``'s Philox draws, ``Diffusion.sampling_ddim`` against its float64 restatement
(``tests/_ddim_ref.py``) around ``UNetOracle``, its two anchors to the existing ``sampling`` (one step bit for bit; the full
sequence at eta = 1), graph replay against eager launches over a chunked visited-step FiLM table, determinism and sharding,
the interpolation modes, model state, errors and the driver.

Bar of the trajectories: 1e-4 max-norm relative, the project's split-bf16 bar for short trajectories
(``tests/test_gpu_samplers.py``)."""
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ddpm_oracle as D  # noqa: E402
from oracle import unet_oracle as U  # noqa: E402
from tests import _ddim_ref as R  # noqa: E402
from tests._common import SMALL, make_args, max_rel  # noqa: E402
from worddiffusion_amd import Diffusion, UNetModel, UNetModelPhosc  # noqa: E402
from worddiffusion_amd import _native as N  # noqa: E402
from worddiffusion_amd.diffusion import draw_style_pairs  # noqa: E402
from worddiffusion_amd.synthetic import fill_module_, synthetic_tensor  # noqa: E402

DEV = "cuda:0"
HW = (32, 64)
CFG339 = dict(SMALL, num_classes=339)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _model(cls, cfg, seed, **args_kw):
    return fill_module_(cls(args=make_args(device=DEV, **args_kw), **cfg), seed).to(DEV).eval()


def _ddim_step(x, eps, tabs, k_dev, t_dev, second=None, scale=0.0, eps_out=None, noise=None, seed=0, offset=0):
    lib = N.lib()
    batch, n = x.shape[0], x[0].numel()
    return lib.wd_ddim_step(x.data_ptr(), eps.data_ptr(), None if second is None else second.data_ptr(), float(scale),
                            None if eps_out is None else eps_out.data_ptr(), batch, n, *(c.data_ptr() for c in tabs),
                            k_dev.data_ptr(), t_dev.data_ptr(), None if noise is None else noise.data_ptr(), seed, offset, _st())


# ------------------------------------------------------------------------------------------------ 1. kernel against torch
@pytest.mark.parametrize("eta", [0.0, 1.0])
@pytest.mark.parametrize("scale", [None, 3.0, 0.3])
def test_ddim_step_kernel_bit_equal_to_unfused_torch(eta, scale):
    lib = N.lib()
    d = Diffusion(noise_steps=1000)
    tau = d.ddim_timesteps(3)
    assert tau == [999, 500, 1]
    S = len(tau)
    tabs = d._ddim_tables(tau, eta, DEV)
    c1, c2, c3, c4, c5 = tabs
    g = torch.Generator().manual_seed(11)
    x, first, second, z = (torch.randn(5, 4, 8, 32, generator=g).to(DEV) for _ in range(4))
    assert x[0].numel() == 1024
    tau_dev = torch.tensor(tau, dtype=torch.int32, device=DEV)
    k_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    t_dev = torch.tensor([tau[0]], dtype=torch.int32, device=DEV)
    t64 = torch.zeros(5, dtype=torch.int64, device=DEV)
    eps_out = torch.zeros_like(x)
    xk = x.clone()
    ref = x.clone()
    for k in range(S):
        N.check(_ddim_step(xk, first, tabs, k_dev, t_dev, second=second if scale is not None else None, scale=scale or 0.0,
                           eps_out=eps_out, noise=z), "wd_ddim_step")
        # the same expression, one torch op per arithmetic operation (nothing for torch to fuse)
        e = first if scale is None else torch.lerp(second, first, scale)
        prod = c1[k] * e
        diff = ref - prod
        x0 = diff * c2[k]
        mean = c3[k] * x0
        direction = c4[k] * e
        ref = mean + direction
        if float(c5[k]) != 0.0:
            zs = c5[k] * z
            ref = ref + zs
        torch.cuda.synchronize()
        assert torch.equal(eps_out, e), (k, "eps_out")
        assert torch.equal(xk, ref), k
        N.check(lib.wd_next_timestep(k_dev.data_ptr(), tau_dev.data_ptr(), S, t_dev.data_ptr(), t64.data_ptr(), 5, _st()),
                "wd_next_timestep")
        kn = min(k + 1, S - 1)
        assert int(k_dev.item()) == kn and int(t_dev.item()) == tau[kn]
        assert torch.equal(t64.cpu(), torch.full((5,), tau[kn], dtype=torch.int64))
    # (the S-th call above already held k at S - 1; once more)
    N.check(lib.wd_next_timestep(k_dev.data_ptr(), tau_dev.data_ptr(), S, t_dev.data_ptr(), t64.data_ptr(), 5, _st()), "wd_next_timestep")
    assert int(k_dev.item()) == S - 1 and int(t_dev.item()) == tau[-1] and bool((t64 == tau[-1]).all())
    assert torch.isfinite(xk).all()


def test_ddim_step_rejects_bad_arguments():
    lib = N.lib()
    tabs = Diffusion(noise_steps=8)._ddim_tables([7, 4, 1], 1.0, DEV)
    k_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    t_dev = torch.tensor([7], dtype=torch.int32, device=DEV)
    buf = torch.zeros(2 * 1024 + 8, device=DEV)
    x, eps = torch.zeros(2, 1024, device=DEV), torch.zeros(2, 1024, device=DEV)
    off = buf[1:1 + 2048].view(2, 1024)  # 4 bytes past a 16-byte boundary
    assert off.data_ptr() % 16 == 4
    assert _ddim_step(x, eps, tabs, k_dev, t_dev) == N.WD_OK
    for kw in (dict(noise=off), dict(second=off)):
        assert _ddim_step(x, eps, tabs, k_dev, t_dev, **kw) == N.WD_EINVAL
    assert _ddim_step(off, eps, tabs, k_dev, t_dev) == N.WD_EINVAL and _ddim_step(x, off, tabs, k_dev, t_dev) == N.WD_EINVAL
    assert _ddim_step(x.view(2, 1024)[:, :1022].contiguous(), eps, tabs, k_dev, t_dev) == N.WD_EINVAL  # n_per_sample % 4
    args = [x.data_ptr(), eps.data_ptr(), None, 0.0, None, 2, 1024] + [c.data_ptr() for c in tabs] + \
        [k_dev.data_ptr(), t_dev.data_ptr(), None, 0, 0, _st()]
    for null in (0, 1, 7, 11, 12, 13):
        bad = list(args)
        bad[null] = None
        assert lib.wd_ddim_step(*bad) == N.WD_EINVAL, null
    t64 = torch.zeros(2, dtype=torch.int64, device=DEV)
    tau_dev = torch.tensor([7, 4, 1], dtype=torch.int32, device=DEV)
    assert lib.wd_next_timestep(None, tau_dev.data_ptr(), 3, t_dev.data_ptr(), t64.data_ptr(), 2, _st()) == N.WD_EINVAL
    assert lib.wd_next_timestep(k_dev.data_ptr(), tau_dev.data_ptr(), 0, t_dev.data_ptr(), t64.data_ptr(), 2, _st()) == N.WD_EINVAL
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. Philox path
def test_ddim_step_draws_the_noise_of_the_ddpm_step():
    lib = N.lib()
    n, seed, row0, batch = 4 * 4 * 8, 77, 6, 3
    one, zero = torch.ones(1, device=DEV), torch.zeros(1, device=DEV)
    k_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    ones_T, zeros_T = torch.ones(12, device=DEV), torch.zeros(12, device=DEV)
    eps = torch.zeros(batch, n, device=DEV)
    for t in (11, 5, 2):
        t_dev = torch.tensor([t], dtype=torch.int32, device=DEV)
        x = torch.zeros(batch, n, device=DEV)
        N.check(_ddim_step(x, eps, (zero, zero, zero, zero, one), k_dev, t_dev, seed=seed, offset=row0), "wd_ddim_step")
        # what wd_ddpm_step adds for the same (seed, row, t): x = eps = 0, ca = 1, cb = 0, cs = 1
        for b in range(batch):
            xr = torch.zeros(1, n, device=DEV)
            N.check(lib.wd_ddpm_step(xr.data_ptr(), eps.data_ptr(), 1, n, ones_T.data_ptr(), zeros_T.data_ptr(), ones_T.data_ptr(),
                                     t_dev.data_ptr(), None, seed, row0 + b, _st()), "wd_ddpm_step")
            torch.cuda.synchronize()
            assert torch.equal(x[b], xr[0]), (t, b)
        assert float(x.std()) > 0.5
    # c5[k] == 0: the term is omitted - a buffer of NaNs is never read, nor multiplied by zero
    nan = torch.full((batch, n), float("nan"), device=DEV)
    x = torch.ones(batch, n, device=DEV)
    N.check(_ddim_step(x, eps, (zero, one, one, zero, zero), k_dev, t_dev, noise=nan), "wd_ddim_step")
    torch.cuda.synchronize()
    assert torch.isfinite(x).all() and torch.equal(x, torch.ones_like(x))


# ------------------------------------------------------------------------------------------------ 3. trajectory against the oracle
@pytest.mark.parametrize("variant", ["base", "phosc"])
@pytest.mark.parametrize("eta", [0.0, 0.7])
def test_ddim_trajectory_matches_float64_oracle(variant, eta):
    T, S, n, seed = 8, 4, 3, 9
    phosc_on = variant == "phosc"
    args = make_args(device=DEV, phosc=1 if phosc_on else 0)
    m = _model(UNetModelPhosc if phosc_on else UNetModel, SMALL, seed, phosc=1 if phosc_on else 0)
    diff = Diffusion(noise_steps=T, img_size=HW, args=args)
    assert diff.ddim_timesteps(S) == [7, 5, 3, 1]
    g = torch.Generator().manual_seed(3)
    x_T = torch.randn(n, 4, 4, 8, generator=g)
    noise = [torch.randn(n, 4, 4, 8, generator=g) for _ in range(S)]
    labels = torch.tensor([1, 7, 10], dtype=torch.int64)
    word = "Moving"
    ph = torch.randint(0, 2, (n, 37), generator=g) if phosc_on else None
    rec = []
    out = diff.sampling_ddim(m, None, n, word, labels, args, steps=S, eta=eta, x_T=x_T, noise=noise, record=rec, phoscLabels=ph)
    st = diff.last_stats
    assert st["sampler"] == "ddim" and st["steps"] == S and st["eta"] == eta and st["timesteps"] == [7, 5, 3, 1]
    assert st["model_calls"] == S and st["forwards_per_step"] == 1
    sd = {k: torch.from_numpy(synthetic_tensor(k, s, seed)).double() for k, s in U.state_dict_shapes(SMALL, variant)}
    orc = U.UNetOracle(SMALL, sd, variant, phosc_on)
    ctx = torch.tensor([D.label_padding(word)] * n, dtype=torch.int64)
    ref_rec = []
    with torch.no_grad():
        ref = R.sampling(lambda x, t: orc(x, t, ctx, labels, ph), x_T, T, [7, 5, 3, 1], eta, noise, record=ref_rec)
    xs = torch.stack([r.cpu() for r in rec] + [out.cpu()])
    ref_xs = torch.stack(ref_rec + [ref])
    assert xs.shape == ref_xs.shape == (S + 1, n, 4, 4, 8)
    errs = [max_rel(xs[k], ref_xs[k]) for k in range(S + 1)]
    print(f"ddim trajectory {variant} eta {eta}: max_rel per state {['%.2e' % e for e in errs]}")
    assert max(errs) < 1e-4
    # the graph replay (no recording) gives the recorded eager run's bits
    again = diff.sampling_ddim(m, None, n, word, labels, args, steps=S, eta=eta, x_T=x_T, noise=noise, phoscLabels=ph)
    assert diff.last_stats["graph"] and torch.equal(again, out)


# ------------------------------------------------------------------------------------------------ 4. / 5. anchors to ``sampling``
def test_one_ddim_step_on_the_prediction_of_the_existing_sampler():
    T, n = 8, 3
    args = make_args(device=DEV)
    m = _model(UNetModel, SMALL, 4)
    diff = Diffusion(noise_steps=T, img_size=HW, args=args)
    X = torch.randn(n, 4, 4, 8, generator=torch.Generator().manual_seed(8))
    labels = torch.tensor([0, 5, 9], dtype=torch.int64)
    preds = []
    diff.sampling(m, None, n, "anchor", labels, args, x_T=X, seed=1, record_pred=preds)
    eps = preds[0][0]
    got = diff.sampling_ddim(m, None, n, "anchor", labels, args, steps=1, eta=0, x_T=X)
    assert diff.last_stats["timesteps"] == [T - 1]
    c1, c2, c3, c4, c5 = (c[0] for c in diff._ddim_tables([T - 1], 0.0, DEV))
    Xd = X.to(DEV)
    prod = c1 * eps
    d = Xd - prod
    x0 = d * c2
    mean = c3 * x0
    direction = c4 * eps
    want = mean + direction
    assert torch.equal(got, want)


def test_full_sequence_eta1_zero_noise_equals_existing_sampler():
    T, n = 8, 3
    args = make_args(device=DEV)
    m = _model(UNetModel, SMALL, 4)
    diff = Diffusion(noise_steps=T, img_size=HW, args=args)
    X = torch.randn(n, 4, 4, 8, generator=torch.Generator().manual_seed(8))
    labels = torch.tensor([0, 5, 9], dtype=torch.int64)
    zero = torch.zeros_like(X)
    ddpm = diff.sampling(m, None, n, "anchor", labels, args, x_T=X, noise=[zero] * (T - 2))
    ddim = diff.sampling_ddim(m, None, n, "anchor", labels, args, steps=T - 1, eta=1.0, x_T=X, noise=[zero] * (T - 1))
    err = max_rel(ddim.cpu(), ddpm.cpu())
    print(f"ddim(S = T-1, eta = 1, zero noise) against sampling(zero noise): max_rel {err:.3e}")
    assert err < 1e-4


# ------------------------------------------------------------------------------------------------ 6. graph == eager, FiLM table
def test_graph_replay_equals_eager_over_a_chunked_visited_step_table(monkeypatch):
    from worddiffusion_amd import engine
    T, S, n = 12, 6, 3
    args = make_args(device=DEV)
    labels = torch.tensor([4, 5, 6], dtype=torch.int64)
    diff = Diffusion(noise_steps=T, img_size=HW, args=args)
    kw = dict(steps=S, eta=0.5, seed=21)
    whole = _model(UNetModel, SMALL, 9)
    default = diff.sampling_ddim(whole, None, n, "text", labels, args, **kw)
    Pw = next(iter(whole.engine._plans.values()))
    assert Pw.film_nchunks == 1 and Pw.film_chunk == S  # the table holds the S visited steps, not the T of the schedule
    monkeypatch.setattr(engine, "FILM_CHUNK_ROWS", 8)
    m = _model(UNetModel, SMALL, 9)
    outs = []
    for use_graph in (True, False):
        outs.append(diff.sampling_ddim(m, None, n, "text", labels, args, use_graph=use_graph, **kw))
        assert diff.last_stats["graph"] == use_graph
    P = next(iter(m.engine._plans.values()))
    assert P.film_chunk * n <= 8 and P.film_nchunks == -(-S // P.film_chunk) and P.film_nchunks > 1  # cut from S * B rows
    assert P.film_table.shape[0] == P.film_chunk * n
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0], default)
    assert torch.isfinite(default).all() and float(default.std()) > 0
    # without the table (time MLP + emb_layers inside every step): graph == eager as well, and the tabulated result to the bar
    # ``test_film_table_chunks_equal_the_per_step_path`` holds the same two paths to under ``sampling``
    diff.tabulate_film = False
    mp = _model(UNetModel, SMALL, 9)
    per_step = [diff.sampling_ddim(mp, None, n, "text", labels, args, use_graph=g, **kw) for g in (True, False)]
    assert getattr(next(iter(mp.engine._plans.values())), "film_nchunks", 0) == 0 and not diff.last_stats["graph"]
    assert torch.equal(per_step[0], per_step[1])
    err = max_rel(per_step[0].cpu(), default.cpu())
    print(f"ddim without the FiLM table against the tabulated result: max_rel {err:.3e}")
    assert err < 1e-5


# ------------------------------------------------------------------------------------------------ 7. determinism and sharding
def test_eta0_is_deterministic_and_noise_is_keyed_by_the_global_row():
    T, S = 10, 4
    args = make_args(device=DEV)
    m = _model(UNetModel, SMALL, 12)
    diff = Diffusion(noise_steps=T, img_size=HW, args=args)
    labels = torch.tensor([1, 2, 3, 4, 5], dtype=torch.int64)
    words = ["one", "two", "three", "four", "five"]
    X = torch.randn(5, 4, 4, 8, generator=torch.Generator().manual_seed(2))
    a = diff.sampling_ddim(m, None, 5, words, labels, args, steps=S, eta=0.0, x_T=X, seed=1)
    b = diff.sampling_ddim(m, None, 5, words, labels, args, steps=S, eta=0.0, x_T=X, seed=2)
    assert torch.equal(a, b)
    c = diff.sampling_ddim(m, None, 5, words, labels, args, steps=S, eta=0.7, x_T=X, seed=1)
    e = diff.sampling_ddim(m, None, 5, words, labels, args, steps=S, eta=0.7, x_T=X, seed=2)
    assert not torch.equal(c, a) and not torch.equal(c, e)
    # x_T and every step's draw from the Philox stream: rows 2..4 of five, and the same rows as a call of their own
    full = diff.sampling_ddim(m, None, 5, words, labels, args, steps=S, eta=0.7, seed=5)
    part = diff.sampling_ddim(m, None, 3, words[2:], labels[2:], args, steps=S, eta=0.7, seed=5, sample_offset=2)
    print(f"ddim rows 2..4 of n = 5 against n = 3 at sample_offset 2: max_rel {max_rel(part.cpu(), full[2:].cpu()):.3e}")
    assert torch.equal(full[2:], part)


# ------------------------------------------------------------------------------------------------ 8. interpolation
def test_ddim_interpolation_modes():
    T, S, n = 9, 4, 3
    labels = torch.tensor([4, 5, 6], dtype=torch.int64)
    # fixed pairs, a mix rate per sample: one forward per step
    args = make_args(device=DEV)
    m = _model(UNetModelPhosc, CFG339, 9)
    diff = Diffusion(noise_steps=T, img_size=HW, args=args)
    rates = torch.tensor([0.0, 0.5, 1.0])
    random.seed(1)
    state = random.getstate()
    a = diff.sampling_ddim(m, None, n, "text", labels, args, steps=S, seed=21, mix_rate=rates, style_pairs=(3, 7))
    assert diff.last_stats["forwards_per_step"] == 1 and diff.last_stats["model_calls"] == S
    assert random.getstate() == state
    b = diff.sampling_ddim(m, None, n, "text", labels, args, steps=S, seed=21, mix_rate=rates, style_pairs=(5, 6))
    assert torch.isfinite(a).all() and not torch.equal(a, b)
    # m = 0 blends nothing: sample 0 is writer 3's
    plain = diff.sampling_ddim(m, None, n, "text", torch.tensor([3, 3, 3]), args, steps=S, seed=21)
    assert torch.equal(plain[0], a[0]) and not torch.equal(plain[2], a[2])
    # reference mode: every forward draws a pair; cfg_scale > 0 runs both forwards and the guided update
    iargs = make_args(device=DEV, interpolation=True)
    mi = _model(UNetModelPhosc, CFG339, 9, interpolation=True)
    random.seed(31)
    preds = []
    g = diff.sampling_ddim(mi, None, n, "text", labels, iargs, steps=S, seed=21, mix_rate=0.37, cfg_scale=3, record_pred=preds)
    after = random.getstate()
    assert diff.last_stats["forwards_per_step"] == 2 and diff.last_stats["model_calls"] == 2 * S
    random.seed(31)
    pairs = draw_style_pairs(2 * S)
    assert random.getstate() == after
    assert len(preds) == S and all(torch.equal(p[2], torch.lerp(p[1], p[0], 3.0)) for p in preds)
    assert not torch.equal(preds[0][0], preds[0][1]) and pairs[0] != pairs[1]
    random.seed(31)
    assert torch.equal(diff.sampling_ddim(mi, None, n, "text", labels, iargs, steps=S, seed=21, mix_rate=0.37, cfg_scale=3), g)
    random.seed(31)
    one = diff.sampling_ddim(mi, None, n, "text", labels, iargs, steps=S, seed=21, mix_rate=0.37, cfg_scale=0)
    assert diff.last_stats["forwards_per_step"] == 1 and not torch.equal(one, g)
    random.seed(31)
    draw_style_pairs(S)
    after1 = random.getstate()
    random.seed(31)
    diff.sampling_ddim(mi, None, n, "text", labels, iargs, steps=S, seed=21, mix_rate=0.37, cfg_scale=0)
    assert random.getstate() == after1


# ------------------------------------------------------------------------------------------------ 9. model state and errors
def test_ddim_model_state_and_errors():
    T = 8
    args = make_args(device=DEV)
    m = _model(UNetModel, SMALL, 4)
    diff = Diffusion(noise_steps=T, img_size=HW, args=args)
    labels = torch.tensor([0, 5], dtype=torch.int64)
    assert not m.training
    out = diff.sampling_ddim(m, None, 2, "ab", labels, args, steps=3)
    assert m.training and out.shape == (2, 4, 4, 8) and torch.isfinite(out).all()
    for bad in (T, T + 5, 0):
        with pytest.raises(ValueError):
            diff.sampling_ddim(m, None, 2, "ab", labels, args, steps=bad)
    with pytest.raises(ValueError):
        diff.sampling_ddim(m, None, 2, "ab", labels, args, timesteps=[3, 5])
    with pytest.raises(ValueError):
        diff.sampling_ddim(m, None, 2, "ab", labels, args, steps=3, eta=1.0, noise=[torch.zeros(2, 4, 4, 8)])  # one per step
    with pytest.raises(N.NativeError):
        diff.sampling_ddim(m, None, 2, "ab", labels, make_args(device="cpu"), steps=3)
    explicit = diff.sampling_ddim(m, None, 2, "ab", labels, args, timesteps=[7, 4, 1], seed=3)
    assert diff.last_stats["timesteps"] == [7, 4, 1] and diff.last_stats["steps"] == 3
    assert torch.equal(explicit, diff.sampling_ddim(m, None, 2, "ab", labels, args, steps=3, seed=3))  # [7, 4, 1] is steps=3 of T = 8


# ------------------------------------------------------------------------------------------------ 10. driver
def test_driver_command_line_with_the_ddim_sampler(golden_dir, tmp_path, monkeypatch):
    from worddiffusion_amd import driver
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    gt = tmp_path / "gt.txt"
    lines = [ln for ln in open(os.path.join(golden_dir, "gt_samples.txt")).read().splitlines() if ln.strip()]
    gt.write_text("\n".join([ln for ln in lines if not ln.startswith("#")][:3]) + "\n")
    rows = driver.read_gt(str(gt))
    assert len(rows) == 3
    args = make_args(device=DEV)
    kw = dict(image_size=(64, 256), in_channels=4, model_channels=64, out_channels=4, num_res_blocks=1, attention_resolutions=(1, 1),
              channel_mult=(1, 1), num_heads=2, num_classes=339, context_dim=64, vocab_size=53, max_seq_len=10)
    m = fill_module_(UNetModel(args=args, **kw), 17)
    os.makedirs(tmp_path / "run" / "models")
    torch.save(m.state_dict(), tmp_path / "run" / "models" / "ema_ckpt.pt")
    out = tmp_path / "out"
    driver.main(["--gt_train", str(gt), "--models_path", str(tmp_path / "run"), "--save_path", str(out), "--writer_dict",
                 str(tmp_path / "writers.json"), "--batch_size", "2", "--emb_dim", "64", "--num_heads", "2", "--noise_steps", "11",
                 "--seed", "5", "--sampler", "ddim", "--ddim_steps", "4", "--eta", "0.5"])
    assert sorted(os.listdir(out / "images")) == sorted(r[1] + ".npy" for r in rows)
    m = m.to(DEV).eval().requires_grad_(False)
    diff = Diffusion(noise_steps=11, img_size=(64, 256), args=args)
    wr = driver.writer_dict(rows, str(tmp_path / "writers.json"))
    for b0 in (0, 2):  # the driver's batches of 2: rows 0-1, row 2
        chunk = rows[b0:b0 + 2]
        labels = torch.tensor([wr[s] for s, _, _ in chunk], dtype=torch.int64)
        ref = diff.sampling_ddim(m, None, len(chunk), [w for _, _, w in chunk], labels, args, steps=4, eta=0.5, seed=5,
                                 sample_offset=b0).cpu()
        assert diff.last_stats["timesteps"] == [10, 7, 4, 1]
        for (_, image, _), r in zip(chunk, ref):
            assert np.array_equal(np.load(out / "images" / f"{image}.npy"), r.numpy()), image
