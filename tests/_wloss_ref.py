"""numpy specification of wd_weighted_mse_loss (include/wdiff_hip.h; DESIGN.md "Weighted training loss"): the fp32 steps are the
kernel's, one rounding each; the two sums per sample run in float64 in plain ascending order.  The kernel adds in another fixed
order, so the GPU tests hold ``grad`` to the bits only where the sums are exact in any order (masks of k/256) and the losses to one
fp32 ulp.  No GPU, no library."""
import numpy as np


def bin_of(t, nbins, T):
    """The histogram bin of timestep t: (t * nbins) / T in integers."""
    return (int(t) * int(nbins)) // int(T)


def hist_update(hist, sample_loss, live, t, T):
    """The recurrence of the specification applied in place to hist (float64 [nbins][2] = (sum, count)): for b ascending, a sample
    with M_b != 0 adds its rounded fp32 loss and 1 to its bin.  Returns hist."""
    nbins = hist.shape[0]
    for b in range(len(sample_loss)):
        if live[b]:
            k = bin_of(t[b], nbins, T)
            hist[k, 0] = hist[k, 0] + np.float64(np.float32(sample_loss[b]))
            hist[k, 1] = hist[k, 1] + 1.0
    return hist


def weighted_mse(pred, target, mask=None, t=None, weights=None, hist=None, T=None):
    """pred, target [, mask]: float32 [B][n]; t: int [B]; weights: float32 [T] or None; hist: float64 [nbins][2] or None (a copy
    is updated).  Returns dict(grad fp32 [B][n], loss fp32 scalar, sample_loss fp32 [B], live bool [B], hist or None, c fp32 [B])."""
    pred, target = np.asarray(pred, np.float32), np.asarray(target, np.float32)
    B, n = pred.shape
    d = pred - target  # fp32
    if mask is not None:
        mask = np.asarray(mask, np.float32)
    grad = np.zeros((B, n), np.float32)
    sample_loss = np.zeros(B, np.float32)
    live = np.zeros(B, bool)
    c = np.zeros(B, np.float32)
    total = np.float64(0.0)
    with np.errstate(all="ignore"):
        for b in range(B):
            dd = d[b].astype(np.float64) * d[b].astype(np.float64)
            if mask is None:
                M, terms = np.float64(n), dd
            else:
                m64 = mask[b].astype(np.float64)
                M = np.float64(0.0)
                for v in m64:
                    M = M + v
                terms = m64 * dd
            S = np.float64(0.0)
            for v in terms:
                S = S + v
            if M == 0.0:
                continue  # contributes nothing: loss 0, gradient row 0, not in the histogram
            live[b] = True
            w = np.float32(1.0) if weights is None else np.float32(weights[int(t[b])])
            q = S / M
            sample_loss[b] = np.float32(q)
            c[b] = np.float32(2.0 * np.float64(w) / (np.float64(B) * M))
            grad[b] = c[b] * d[b] if mask is None else c[b] * (mask[b] * d[b])
            total = total + np.float64(w) * q
    out_hist = None
    if hist is not None:
        out_hist = hist_update(np.array(hist, np.float64, copy=True), sample_loss, live, t, T)
    return dict(grad=grad, loss=np.float32(total / np.float64(B)), sample_loss=sample_loss, live=live, hist=out_hist, c=c)


def ulp_distance(a, b):
    """Distance between fp32 values in units in the last place (finite, same-sign or zero inputs)."""
    a, b = np.atleast_1d(np.asarray(a, np.float32)), np.atleast_1d(np.asarray(b, np.float32))
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return np.abs(ia - ib)
