"""Host side of the DDIM sampler: the visited-timestep schedule, the coefficient tables against their float64 restatement
(``tests/_ddim_ref.py``), the identity with the reference-pinned DDPM update at S = T-1, eta = 1, what every sampler's description hands the one
reverse loop, the bound symbols and the driver's command line.  No GPU."""
import numpy as np
import pytest
import torch

from oracle import ddpm_oracle as D
from tests import _ddim_ref as R
from worddiffusion_amd import Diffusion
from worddiffusion_amd import _native as N


@pytest.mark.parametrize("T,S", [(1000, 50), (8, 4), (8, 7), (600, 599), (1000, 2), (1000, 1)])
def test_ddim_timesteps_subsequence(T, S):
    tau = Diffusion(noise_steps=T).ddim_timesteps(S)
    assert isinstance(tau, list) and len(tau) == S and all(isinstance(t, int) for t in tau)
    assert all(a > b for a, b in zip(tau, tau[1:]))
    assert tau[0] == T - 1 and (tau[-1] == 1 or S == 1)
    assert tau == R.timesteps(T, S)
    if S == T - 1:
        assert tau == list(range(T - 1, 0, -1))


def test_ddim_timesteps_errors_and_explicit_lists():
    d = Diffusion(noise_steps=8)
    assert d.ddim_timesteps(4) == [7, 5, 3, 1]
    for bad in (0, 8, -3, 100):
        with pytest.raises(ValueError):
            d.ddim_timesteps(bad)
    assert d.ddim_timesteps(timesteps=[6, 4, 1]) == [6, 4, 1]
    assert d.ddim_timesteps(50, timesteps=(7,)) == [7]
    for bad in ([3, 5], [5, 5, 1], [7, 0], [8, 3], [], [4, -1]):
        with pytest.raises(ValueError):
            d.ddim_timesteps(timesteps=bad)


@pytest.mark.parametrize("T,S", [(1000, 50), (8, 4), (8, 7), (600, 599), (1000, 1)])
@pytest.mark.parametrize("eta", [0.0, 0.7, 1.0])
def test_ddim_tables_are_the_float64_values_rounded_once(T, S, eta):
    d = Diffusion(noise_steps=T)
    tau = d.ddim_timesteps(S)
    got = d._ddim_tables(tau, eta, "cpu")
    ref = R.tables(T, tau, eta)
    assert len(got) == 5
    for j, c in enumerate(got):
        assert c.dtype == torch.float32 and c.shape == (S,)
        assert np.array_equal(c.numpy().view(np.int32), ref[j].float().numpy().view(np.int32)), j
    if eta == 0.0:
        assert not got[4].any()
    else:
        assert (got[4] > 0).all()
    ah = R.alpha_hat64(T)
    p = ah[tau[1:] + [0]]
    assert float((got[3].double() ** 2 + got[4].double() ** 2 - (1 - p)).abs().max()) < 1e-6
    assert float(p[-1]) < 1.0  # the last predecessor is alpha_hat[0] of the schedule, not 1


@pytest.mark.parametrize("T", [8, 1000])
def test_full_sequence_eta1_is_the_ddpm_mean(T):
    """S = T-1, eta = 1: c3 ((x - c1 e) c2) + c4 e, evaluated in fp32 in the kernel's order, against the DDPM mean of
    ``oracle.ddpm_oracle.reverse_step`` (z = None) restated in float64 - every t, < 1e-5 max-norm relative."""
    d = Diffusion(noise_steps=T)
    tau = d.ddim_timesteps(T - 1)
    c1, c2, c3, c4, c5 = d._ddim_tables(tau, 1.0, "cpu")
    beta = D.schedule(T)[0].double()  # the reference's fp32 betas; alpha and its cumprod in float64, as the tables take them
    alpha = 1.0 - beta
    ah = torch.cumprod(alpha, dim=0)
    g = torch.Generator().manual_seed(5)
    x, e = torch.randn(1, 4, 8, 128, generator=g), torch.randn(1, 4, 8, 128, generator=g)
    assert x.numel() == 4096
    worst = 0.0
    for k, t in enumerate(tau):
        got = c3[k] * ((x - c1[k] * e) * c2[k]) + c4[k] * e
        assert got.dtype == torch.float32
        ref = D.reverse_step(beta, alpha, ah, x.double(), e.double(), t, torch.zeros_like(x, dtype=torch.float64))
        assert ref.dtype == torch.float64
        worst = max(worst, float((got.double() - ref).abs().max() / ref.abs().max()))
    print(f"DDIM(S = T-1, eta = 1) against the DDPM mean, T = {T}: max_rel {worst:.3e}")
    assert worst < 1e-5


def test_visited_steps_restate_the_reference_loops():
    """``Diffusion._ddpm`` / ``_ddim`` describe the steps the one reverse loop visits - (film_prepare argument, calls the model,
    entry of ``noise`` or None) - against the loops themselves, written out: train.py:221-236 (``for i in reversed(range(1,
    T))``, a fresh ``randn`` while i > 1), regenerateFromtrain2.py:532-620 (the same loop, the model behind the predicate of
    :536, the draw made on every step) and the DDIM loop over tau (a draw only where sigma != 0)."""
    T = 12
    d = Diffusion(noise_steps=T)

    def ddpm_loop(calls):
        want, drawn = [], 0
        for i in reversed(range(1, T)):
            z = None
            if i > 1:
                z, drawn = drawn, drawn + 1
            want.append((i, calls(i), z))
        return want

    s = d._ddpm()
    assert s.steps == ddpm_loop(lambda i: True) and (s.t_first, s.tau) == (11, None)
    assert [a for a, _, _ in s.steps] == list(range(11, 0, -1)) and all(f for _, f, _ in s.steps)
    assert [z for _, _, z in s.steps] == list(range(10)) + [None]
    s3 = d._ddpm(lambda i: Diffusion.sampling3_calls_model(i, T, 0), deterministic=True)
    assert s3.steps == ddpm_loop(lambda i: Diffusion.sampling3_calls_model(i, T, 0)) and (s3.t_first, s3.tau) == (11, None)
    assert [a for a, f, _ in s3.steps if f] == [11, 10, 5]
    assert [z for _, _, z in s3.steps] == list(range(10)) + [None]  # counted on the skipped steps too
    assert s.stats == s3.stats == dict(steps=T - 1)  # the updates, not the model calls
    # the pairs of an interpolating call are drawn for the model-calling steps of that same list, in loop order
    import random
    import types
    from worddiffusion_amd.diffusion import draw_style_pairs
    random.seed(5)
    tab, _, _ = d._mix_setup(types.SimpleNamespace(interpolation=True), 2, 0.37, None, 0, sampler=s3)
    after = random.getstate()
    random.seed(5)
    pairs = draw_style_pairs(3)
    assert random.getstate() == after and tab.shape == (1, T, 2, 2)
    assert [tuple(tab[0, i, 0].tolist()) for i in (11, 10, 5)] == pairs and not tab[0, [9, 8, 7, 6, 4, 3, 2, 1, 0]].any()

    d8 = Diffusion(noise_steps=8)
    tau = [7, 4, 1]
    for eta in (0.0, 1.0):
        c5 = d8._ddim_tables(tau, eta, "cpu")[4]
        want = []
        for j in range(len(tau)):
            want.append((j, True, j if float(c5[j]) != 0 else None))
        sd = d8._ddim(tau, eta)
        assert sd.steps == want and (sd.t_first, sd.tau) == (7, tau)
        assert sd.stats == dict(sampler="ddim", steps=3, eta=eta, timesteps=tau)
        if eta == 0.0:
            assert [z for _, _, z in sd.steps] == [None] * 3
        else:
            assert [z for _, _, z in sd.steps] == [0, 1, 2]  # sigma > 0 at every step, the last (predecessor: index 0) included


def test_ddim_symbols_are_declared_and_bound():
    for name in ("wd_ddim_step", "wd_next_timestep"):
        assert name in N.header_symbols() and name in N._SIGS
    assert len(N._SIGS["wd_ddim_step"][1]) == 18 and len(N._SIGS["wd_next_timestep"][1]) == 7


def test_driver_command_line_sampler_flags():
    from worddiffusion_amd import driver
    base = ["--gt_train", "gt.txt", "--save_path", "out"]
    _, a = driver.parse_args(base)
    assert (a.sampler, a.ddim_steps, a.eta) == ("ddpm", 50, 0.0)
    _, a = driver.parse_args(base + ["--sampler", "ddim", "--ddim_steps", "4", "--eta", "0.5"])
    assert (a.sampler, a.ddim_steps, a.eta) == ("ddim", 4, 0.5)
    for bad in (["--sampler", "ddim", "--skip_steps", "1"], ["--sampler", "plms"],
                ["--sampler", "ddim", "--ddim_steps", "1000"], ["--sampler", "ddim", "--ddim_steps", "0"]):
        with pytest.raises(SystemExit):
            driver.parse_args(base + bad)
    with pytest.raises(ValueError):
        driver.regenerate(None, None, [], {}, None, sampler="plms")
    with pytest.raises(ValueError):
        driver.interpolate(None, None, [], None, (1, 2), sampler="plms")
    with pytest.raises(ValueError):
        driver.regenerate(None, None, [], {}, None, sampler="ddim", skip_steps=True)
