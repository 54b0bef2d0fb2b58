"""Host specification of global-norm gradient clipping as ``FusedAdamW(max_grad_norm=...)`` computes it (numpy, no GPU):

  norm = fp32( sqrt( sum over every gradient element of (double)g * (double)g ) )   - summed in float64, rounded once
  coef = min(1, max_norm / (norm + 1e-6))  in fp32, a NaN quotient staying NaN       - torch.nn.utils.clip_grad_norm_

torch itself takes the norm of the per-tensor fp32 norms, so it agrees with this to fp32 summation error only
(tests/test_clip_accum_host.py holds the two together)."""
import numpy as np


def _np(g):
    return g.detach().cpu().numpy() if hasattr(g, "detach") else np.asarray(g)


def global_norm(grads) -> np.float32:
    """``grads``: iterable of fp32 arrays / tensors (``None`` entries are parameters without a gradient)."""
    total = 0.0
    for g in grads:
        if g is None:
            continue
        a = _np(g)
        assert a.dtype == np.float32
        a = a.astype(np.float64).ravel()
        total += float(np.dot(a, a))
    return np.float32(np.sqrt(np.float64(total)))


def clip_coef(norm, max_norm) -> np.float32:
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        q = np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6))
    if np.isnan(q):
        return np.float32(q)  # torch.clamp(nan, max=1.0) is nan
    return np.float32(min(np.float32(1.0), q))


def clipped(grads, max_norm):
    """(norm, coef, [fp32(g * coef) or None]) - what ``clip_grad_norm_`` leaves in ``.grad``, each product rounded once."""
    norm = global_norm(grads)
    coef = clip_coef(norm, max_norm)
    return norm, coef, [None if g is None else _np(g) * coef for g in grads]
