"""Float64 restatement of the DDIM sampler (Song et al. 2020, eq. 12) on the reference's schedule: the visited timesteps, the
five per-step coefficients and the loop, around a model callable in the manner of ``oracle.ddpm_oracle.sampling``.  A test
helper (not collected): ``tests/test_ddim_host.py`` and ``tests/test_gpu_ddim.py`` compare the product against it."""
import math

import torch


def alpha_hat64(noise_steps=1000, beta_start=1e-4, beta_end=0.02):
    """train.py:180-188 with the fp32 betas of the reference and everything after them in float64."""
    beta = torch.linspace(beta_start, beta_end, noise_steps).double()
    return torch.cumprod(1.0 - beta, dim=0)


def timesteps(noise_steps, steps):
    """``steps`` timesteps from T-1 down to 1, evenly spread in integer arithmetic."""
    T, S = noise_steps, steps
    if not 1 <= S <= T - 1:
        raise ValueError(S)
    if S == 1:
        return [T - 1]
    tau = [1 + ((T - 2) * k) // (S - 1) for k in range(S)]
    return tau[::-1]


def tables(noise_steps, tau, eta):
    """float64 [5, S]: c1 = sqrt(1-a), c2 = 1/sqrt(a), c3 = sqrt(p), c4 = sqrt(max(1-p-sigma^2, 0)), c5 = sigma, with
    a = alpha_hat[tau[k]] and p = alpha_hat[tau[k+1]] (alpha_hat[0] after the last entry: index 0 is never stepped from)."""
    ah = alpha_hat64(noise_steps)
    rows = []
    for k, t in enumerate(tau):
        a = float(ah[t])
        p = float(ah[tau[k + 1]] if k + 1 < len(tau) else ah[0])
        sigma = eta * math.sqrt((1 - p) / (1 - a)) * math.sqrt(1 - a / p)
        rows.append([math.sqrt(1 - a), 1 / math.sqrt(a), math.sqrt(p), math.sqrt(max(1 - p - sigma * sigma, 0.0)), sigma])
    return torch.tensor(rows, dtype=torch.float64).t().contiguous()


def step(c, k, x, eps, z=None):
    """One update with column k of ``tables``; z is used only where sigma != 0."""
    x0 = (x - c[0, k] * eps) * c[1, k]
    x = c[2, k] * x0 + c[3, k] * eps
    if float(c[4, k]) != 0.0:
        x = x + c[4, k] * z
    return x


def sampling(model, x_T, noise_steps, tau, eta=0.0, noises=None, record=None):
    """``model(x, t)`` returns the predicted noise (t int64 [n]); ``noises[k]`` is the draw of visited step k.  Returns x after
    the last step; ``record`` receives the x every step starts from."""
    c = tables(noise_steps, tau, eta)
    x = x_T.double()
    for k, t in enumerate(tau):
        if record is not None:
            record.append(x.clone())
        eps = model(x, torch.full((x.shape[0],), t, dtype=torch.int64)).double()
        x = step(c, k, x, eps, None if noises is None else noises[k].double())
    return x
