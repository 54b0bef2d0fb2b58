"""Host side of the DPM-Solver++(2M) sampler: the visited-timestep schedules, the coefficient tables against their float64
restatement (``tests/_dpmpp_ref.py``), the identity of order 1 with DDIM at eta = 0, the solver's discretisation error on a
target whose probability-flow ODE has a closed-form solution, what the sampler's description hands the one reverse loop, the
bound symbol and the driver's command line.  No GPU."""
import numpy as np
import pytest
import torch

from tests import _dpmpp_ref as R
from worddiffusion_amd import Diffusion
from worddiffusion_amd import _native as N


# ------------------------------------------------------------------------------------------------ 1. timesteps
@pytest.mark.parametrize("T,S", [(1000, 50), (1000, 5), (8, 4), (8, 7), (600, 599), (1000, 999), (1000, 2), (1000, 1)])
def test_dpmpp_timesteps_logsnr(T, S):
    d = Diffusion(noise_steps=T)
    tau = d.dpmpp_timesteps(S)
    assert tau == d.dpmpp_timesteps(S, "logsnr") == d.dpmpp_timesteps(steps=S, spacing="logsnr")
    assert isinstance(tau, list) and len(tau) == S and all(isinstance(t, int) for t in tau)
    assert all(a > b for a, b in zip(tau, tau[1:]))
    assert tau[0] == T - 1 and (tau[-1] == 1 or S == 1)
    assert tau == R.timesteps(T, S, "logsnr")
    if S == T - 1:
        assert tau == list(range(T - 1, 0, -1))
    assert d.dpmpp_timesteps(S, "time") == d.ddim_timesteps(S) == R.timesteps(T, S, "time")


def test_dpmpp_timesteps_pins_errors_and_explicit_lists():
    assert Diffusion(noise_steps=1000).dpmpp_timesteps(5) == [999, 735, 342, 42, 1]
    d = Diffusion(noise_steps=8)
    assert d.dpmpp_timesteps(4) == [7, 4, 2, 1]
    assert R.timesteps(1000, 5) == [999, 735, 342, 42, 1] and R.timesteps(8, 4) == [7, 4, 2, 1]
    for spacing in ("logsnr", "time"):
        for bad in (0, 8, -3, 100):
            with pytest.raises(ValueError):
                d.dpmpp_timesteps(bad, spacing)
    with pytest.raises(ValueError):
        d.dpmpp_timesteps(4, "karras")
    assert d.dpmpp_timesteps(timesteps=[6, 4, 1]) == [6, 4, 1]
    assert d.dpmpp_timesteps(50, timesteps=(7,)) == [7]
    assert d.dpmpp_timesteps(50, "time", timesteps=(7, 2)) == [7, 2]
    for bad in ([3, 5], [5, 5, 1], [7, 0], [8, 3], [], [4, -1]):
        with pytest.raises(ValueError):
            d.dpmpp_timesteps(timesteps=bad)


# ------------------------------------------------------------------------------------------------ 2. tables
@pytest.mark.parametrize("T,S", [(1000, 50), (1000, 20), (8, 4), (8, 7), (600, 599), (1000, 2), (1000, 1)])
@pytest.mark.parametrize("order", [1, 2])
def test_dpmpp_tables_are_the_float64_values_rounded_once(T, S, order):
    d = Diffusion(noise_steps=T)
    tau = d.dpmpp_timesteps(S)
    got = d._dpmpp_tables(tau, order, "cpu")
    ref = R.tables(T, tau, order)
    assert len(got) == 5
    for j, c in enumerate(got):
        assert c.dtype == torch.float32 and c.shape == (S,)
        assert np.array_equal(c.numpy().view(np.int32), ref[j].float().numpy().view(np.int32)), j
    c5 = got[4]
    assert float(c5[0]) == 0.0 and float(c5[-1]) == 0.0
    if order == 1:
        assert not c5.any()
    elif S > 2:
        assert (c5[1:-1] > 0).all()
    ah = R.alpha_hat64(T)
    a, p = ah[tau], ah[tau[1:] + [0]]
    assert float((got[2].double() ** 2 * (1 - a) - (1 - p)).abs().max()) < 1e-6
    assert float(p[-1]) < 1.0  # the last predecessor is alpha_hat[0] of the schedule, not 1
    assert (got[3] > 0).all()  # h > 0 at every step: the log-SNR rises along tau


def test_dpmpp_tables_reject_other_orders():
    d = Diffusion(noise_steps=8)
    for bad in (0, 3, 2.5, None):
        with pytest.raises(ValueError):
            d._dpmpp_tables([7, 4, 1], bad, "cpu")
        with pytest.raises(ValueError):
            d._dpmpp(([7, 4, 1]), bad)


# ------------------------------------------------------------------------------------------------ 3. order 1 is DDIM
@pytest.mark.parametrize("T,S,spacing", [(1000, 50, "logsnr"), (1000, 20, "time"), (8, 4, "logsnr"), (8, 7, "time")])
def test_order1_is_ddim_eta0(T, S, spacing):
    """The first-order update x <- c3 x + c4 x0 is DDIM's sqrt(p) x0 + sqrt(1-p) e with x = sqrt(a) x0 + sqrt(1-a) e
    substituted: both evaluated in fp32 in their kernel's order, every step of the same tau, < 1e-5 max-norm relative."""
    d = Diffusion(noise_steps=T)
    tau = d.dpmpp_timesteps(S, spacing)
    c1, c2, c3, c4, c5 = d._dpmpp_tables(tau, 1, "cpu")
    d1, d2, d3, d4, d5 = d._ddim_tables(tau, 0.0, "cpu")
    assert torch.equal(c1, d1) and torch.equal(c2, d2) and not c5.any() and not d5.any()
    g = torch.Generator().manual_seed(5)
    x, e = torch.randn(1, 4, 8, 128, generator=g), torch.randn(1, 4, 8, 128, generator=g)
    assert x.numel() == 4096
    worst = 0.0
    for k in range(S):
        x0 = (x - c1[k] * e) * c2[k]
        got = c3[k] * x + c4[k] * x0
        ref = d3[k] * ((x - d1[k] * e) * d2[k]) + d4[k] * e
        assert got.dtype == ref.dtype == torch.float32
        worst = max(worst, float((got.double() - ref.double()).abs().max() / ref.double().abs().max()))
    print(f"DPM-Solver++ order 1 against DDIM eta 0, T = {T}, S = {S}, {spacing}: max_rel {worst:.3e}")
    assert worst < 1e-5


# ------------------------------------------------------------------------------------------------ 4. solver accuracy
def _toy_eps(x, ah_t, s2):
    """The exact noise prediction for data ~ N(0, s2 I): sqrt(1-ah) x / (ah s2 + 1 - ah)."""
    return (1 - ah_t) ** 0.5 * x / (ah_t * s2 + 1 - ah_t)


def _toy_errors(T=1000):
    """max-norm relative error, against the exact probability-flow ODE solution from T-1 to index 0, of the product's
    timesteps and (fp32) tables run through a float64 loop of each kernel's formula: {(solver, S, s2): err}."""
    d = Diffusion(noise_steps=T)
    ah = R.alpha_hat64(T)
    x_T = torch.randn(4096, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    out = {}
    for s2 in (1.0, 0.25, 0.03):
        v = ah * s2 + 1 - ah
        exact = x_T * float(v[0] / v[T - 1]) ** 0.5
        for S in (10, 20, 50):
            tau = d.dpmpp_timesteps(S, "logsnr")
            for order in (2, 1):
                c1, c2, c3, c4, c5 = (c.double() for c in d._dpmpp_tables(tau, order, "cpu"))
                x, prev = x_T.clone(), None
                for k, t in enumerate(tau):
                    x0 = (x - c1[k] * _toy_eps(x, float(ah[t]), s2)) * c2[k]
                    D = x0 if float(c5[k]) == 0.0 else x0 + c5[k] * (x0 - prev)
                    x, prev = c3[k] * x + c4[k] * D, x0
                out["2m" if order == 2 else "1", S, s2] = float((x - exact).abs().max() / exact.abs().max())
            tau = d.ddim_timesteps(S)
            c1, c2, c3, c4, c5 = (c.double() for c in d._ddim_tables(tau, 0.0, "cpu"))
            x = x_T.clone()
            for k, t in enumerate(tau):
                e = _toy_eps(x, float(ah[t]), s2)
                x = c3[k] * ((x - c1[k] * e) * c2[k]) + c4[k] * e
            out["ddim", S, s2] = float((x - exact).abs().max() / exact.abs().max())
    return out


def test_solver_error_on_a_gaussian_target():
    """Data ~ N(0, s^2 I): eps*(x, t) = sqrt(1-ah_t) x / v(t), v(t) = ah_t s^2 + 1 - ah_t, and the ODE's exact solution from T-1 to
    index 0 is x_T sqrt(v(0) / v(T-1)).  (a) 2M on log-SNR spacing is at least 3x closer to it than DDIM (eta = 0, its own
    even-in-t timesteps) at S = 10, 20, 50; (b) from S = 20 to S = 50 its error falls by at least 4 (second order: 2.5^2 = 6.25;
    first order would give 2.5).  Figures of this test (T = 1000; 2M log-SNR | order 1 log-SNR | DDIM even-in-t):
        s^2 = 1     S = 10: 3.57e-02 | 2.27e-01 | 1.84e-01    S = 20: 1.36e-02 | 1.15e-01 | 9.11e-02    S = 50: 2.21e-03 | 4.62e-02 | 3.63e-02
        s^2 = 0.25  S = 10: 3.05e-02 | 2.27e-01 | 2.72e-01    S = 20: 1.35e-02 | 1.15e-01 | 1.36e-01    S = 50: 2.18e-03 | 4.63e-02 | 5.50e-02
        s^2 = 0.03  S = 10: 1.16e-02 | 2.27e-01 | 5.24e-01    S = 20: 1.19e-02 | 1.15e-01 | 3.04e-01    S = 50: 1.77e-03 | 4.65e-02 | 1.29e-01
    (worst 2M / DDIM ratio 0.194, at S = 10, s^2 = 1; S = 20 -> 50 improvements 6.2, 6.2, 6.7)"""
    err = _toy_errors()
    for s2 in (1.0, 0.25, 0.03):
        print(f"s^2 = {s2}: " + "    ".join(
            f"S = {S}: {err['2m', S, s2]:.2e} | {err['1', S, s2]:.2e} | {err['ddim', S, s2]:.2e}" for S in (10, 20, 50)))
    for s2 in (1.0, 0.25, 0.03):
        for S in (10, 20, 50):
            assert err["2m", S, s2] <= err["ddim", S, s2] / 3, (S, s2)
        assert err["2m", 50, s2] <= err["2m", 20, s2] / 4, s2


# ------------------------------------------------------------------------------------------------ 5. structure, binding, driver
def test_dpmpp_sampler_description():
    d8 = Diffusion(noise_steps=8)
    tau = [7, 4, 1]
    for order in (1, 2):
        s = d8._dpmpp(tau, order)
        assert s.steps == [(0, True, None), (1, True, None), (2, True, None)] and (s.t_first, s.tau) == (7, tau)
        assert s.tau is not tau  # a copy: the caller's list is not kept
        assert s.stats == dict(sampler="dpmpp", steps=3, order=order, spacing=None, timesteps=tau)
        assert callable(s.update)
    assert d8._dpmpp(d8.dpmpp_timesteps(4), 2, "logsnr").stats == dict(sampler="dpmpp", steps=4, order=2, spacing="logsnr",
                                                                       timesteps=[7, 4, 2, 1])


def test_dpmpp_symbol_is_declared_and_bound():
    assert "wd_dpmpp_step" in N.header_symbols() and "wd_dpmpp_step" in N._SIGS
    assert len(N._SIGS["wd_dpmpp_step"][1]) == 15


def test_driver_command_line_dpmpp_flags():
    from worddiffusion_amd import driver
    base = ["--gt_train", "gt.txt", "--save_path", "out"]
    _, a = driver.parse_args(base)
    assert (a.sampler, a.dpmpp_steps, a.dpmpp_order, a.dpmpp_spacing) == ("ddpm", 20, 2, "logsnr")
    _, a = driver.parse_args(base + ["--sampler", "dpmpp", "--dpmpp_steps", "4", "--dpmpp_order", "1", "--dpmpp_spacing", "time"])
    assert (a.sampler, a.dpmpp_steps, a.dpmpp_order, a.dpmpp_spacing) == ("dpmpp", 4, 1, "time")
    _, a = driver.parse_args(base + ["--sampler", "dpmpp"])
    assert (a.sampler, a.dpmpp_steps, a.dpmpp_order, a.dpmpp_spacing) == ("dpmpp", 20, 2, "logsnr")
    for bad in (["--sampler", "dpmpp", "--dpmpp_steps", "0"], ["--sampler", "dpmpp", "--dpmpp_steps", "1000"],
                ["--sampler", "dpmpp", "--skip_steps", "1"], ["--sampler", "dpmpp", "--dpmpp_order", "3"],
                ["--sampler", "dpmpp", "--dpmpp_spacing", "karras"], ["--sampler", "plms"]):
        with pytest.raises(SystemExit):
            driver.parse_args(base + bad)
    with pytest.raises(ValueError):
        driver.regenerate(None, None, [], {}, None, sampler="dpmpp", skip_steps=True)
    with pytest.raises(ValueError):
        driver.regenerate(None, None, [], {}, None, sampler="plms")
    # no rows: nothing is sampled, the sampler name is accepted
    assert driver.regenerate(None, None, [], {}, None, sampler="dpmpp", rank=0, world=1)[0] == 0
