"""Float64 restatement of the DPM-Solver++(2M) sampler (Lu et al. 2022, algorithm 2) on the reference's schedule: the visited
timesteps (evenly spaced in log-SNR, or in t), the five per-step coefficients and the loop, around a model callable in the
manner of ``tests/_ddim_ref.py``.  Written with scalar ``math`` on Python floats, independently of the product's tensor code.  A
test helper (not collected): ``tests/test_dpmpp_host.py`` and ``tests/test_gpu_dpmpp.py`` compare the product against it."""
import math

import torch


def alpha_hat64(noise_steps=1000, beta_start=1e-4, beta_end=0.02):
    """train.py:180-188 with the fp32 betas of the reference and everything after them in float64."""
    beta = torch.linspace(beta_start, beta_end, noise_steps).double()
    return torch.cumprod(1.0 - beta, dim=0)


def _lam(v):
    """Half the log-SNR of a point with alpha_hat = v."""
    return 0.5 * math.log(v / (1.0 - v))


def timesteps(noise_steps, steps, spacing="logsnr"):
    """``steps`` timesteps from T-1 down to 1: evenly spread in t in integer arithmetic (``"time"``), or each the index whose
    log-SNR is nearest to one of ``steps`` evenly spread targets (``"logsnr"``; the lowest index on a tie), pushed below its
    predecessor and kept high enough for the entries that follow."""
    T, S = noise_steps, steps
    if not 1 <= S <= T - 1:
        raise ValueError(S)
    if S == 1:
        return [T - 1]
    if spacing == "time":
        return [1 + ((T - 2) * k) // (S - 1) for k in range(S)][::-1]
    if spacing != "logsnr":
        raise ValueError(spacing)
    lam = [None] + [_lam(float(v)) for v in alpha_hat64(T)[1:]]
    hi, lo = lam[1], lam[T - 1]
    tau = []
    for k in range(S):
        target = lo + (hi - lo) * k / (S - 1)
        best, best_d = None, None
        for t in range(1, T):  # ascending: a later index replaces the best only when strictly nearer
            d = abs(lam[t] - target)
            if best is None or d < best_d:
                best, best_d = t, d
        if tau:
            best = min(best, tau[-1] - 1)
        tau.append(max(best, S - k))
    return tau


def tables(noise_steps, tau, order):
    """float64 [5, S]: c1 = sqrt(1-a), c2 = 1/sqrt(a), c3 = sqrt((1-p)/(1-a)), c4 = -sqrt(p) expm1(-h), c5 = h_k / (2 h_{k-1}), with
    a = alpha_hat[tau[k]], p = alpha_hat[tau[k+1]] (alpha_hat[0] after the last entry) and h = lambda(p) - lambda(a).  c5 is 0 at
    the first step, at the last one, and everywhere at order 1."""
    if order not in (1, 2):
        raise ValueError(order)
    ah = alpha_hat64(noise_steps)
    S = len(tau)
    rows, h_before = [], None
    for k, t in enumerate(tau):
        a = float(ah[t])
        p = float(ah[tau[k + 1]] if k + 1 < S else ah[0])
        h = _lam(p) - _lam(a)
        second = order == 2 and 0 < k < S - 1
        rows.append([math.sqrt(1 - a), 1 / math.sqrt(a), math.sqrt((1 - p) / (1 - a)), -math.sqrt(p) * math.expm1(-h),
                     h / (2 * h_before) if second else 0.0])
        h_before = h
    return torch.tensor(rows, dtype=torch.float64).t().contiguous()


def step(c, k, x, eps, x0_prev):
    """One update with column k of ``tables``: returns (x, x0).  ``x0_prev`` is used only where c5[k] != 0."""
    x0 = (x - c[0, k] * eps) * c[1, k]
    d = x0
    if float(c[4, k]) != 0.0:
        d = x0 + c[4, k] * (x0 - x0_prev)
    return c[2, k] * x + c[3, k] * d, x0


def sampling(model, x_T, noise_steps, tau, order=2, record=None):
    """``model(x, t)`` returns the predicted noise (t int64 [n]).  Returns x after the last step; ``record`` receives the x every
    step starts from."""
    c = tables(noise_steps, tau, order)
    x = x_T.double()
    x0_prev = None
    for k, t in enumerate(tau):
        if record is not None:
            record.append(x.clone())
        eps = model(x, torch.full((x.shape[0],), t, dtype=torch.int64)).double()
        x, x0_prev = step(c, k, x, eps, x0_prev)
    return x
