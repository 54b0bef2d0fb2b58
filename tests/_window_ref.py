"""Line sampling as overlapping windows (``wd_window_gather`` / ``wd_window_blend``, include/wdiff_hip.h; MultiDiffusion, Bar-Tal et
al. 2023), restated in numpy from its specification and from nothing in the library.  A test helper (not collected).

A line latent ``line[s, c, r, J]`` of width ``Wl`` is denoised as ``K`` windows of width ``w`` per line; window ``k`` of line ``s``
is model batch row ``b = s * K + k`` and begins at column ``o[s, k]``, ``0 <= o <= Wl - w``.  With weights ``weight[s, k, j] >= 0``,

    wn[s, k, j] = weight[s, k, j] / sum_k' weight[s, k', J - o[s, k']],   J = o[s, k] + j,

summed over the windows that cover J, in float64, rounded to fp32 once.  A column is covered when some window has wn > 0 there.

    gather:  win[b, c, r, j] = line[s, c, r, o[s, k] + j]                                     (the bits)
    blend:   over the windows k ascending with o <= J < o + w and wn[s, k, J - o] != 0:
                 acc = wn * e   (the first),   acc = acc + wn * e   (each later one),
             each product and each sum rounded to fp32 on its own; 0.0 where nothing covers.

numpy rounds every fp32 operation once and fuses nothing, which is the rounding the kernels are held to."""
import numpy as np


def profile(w, feather=0):
    """min(j + 1, w - j, feather + 1) / (feather + 1), fp32 [w]: 1 in the middle, a linear ramp of ``feather`` columns at each end."""
    j = np.arange(w, dtype=np.float64)
    return (np.minimum(np.minimum(j + 1, w - j), feather + 1) / (feather + 1)).astype(np.float32)


def _full(offsets, weight, n):
    o = np.asarray(offsets, dtype=np.int64)
    if o.ndim == 1:
        o = np.broadcast_to(o, (n, o.shape[0]))
    K = o.shape[1]
    wt = np.asarray(weight, dtype=np.float32)
    wt = np.broadcast_to(wt, (n, K, wt.shape[-1]))
    return o, wt


def coverage(offsets, weight, width, n=1):
    """The float64 sum of the weights over every line column, [n, width]."""
    o, wt = _full(offsets, weight, n)
    w = wt.shape[-1]
    tot = np.zeros((o.shape[0], width), dtype=np.float64)
    for s in range(o.shape[0]):
        for k in range(o.shape[1]):
            tot[s, o[s, k]:o[s, k] + w] += wt[s, k].astype(np.float64)
    return tot


def normalise(offsets, weight, width, n=1):
    """wn, fp32 [n, K, w]; 0 where the column's sum is 0 (an uncovered column: the host refuses the layout)."""
    o, wt = _full(offsets, weight, n)
    w = wt.shape[-1]
    tot = coverage(o, wt, width, o.shape[0])
    wn = np.zeros(wt.shape, dtype=np.float32)
    for s in range(o.shape[0]):
        for k in range(o.shape[1]):
            t = tot[s, o[s, k]:o[s, k] + w]
            with np.errstate(invalid="ignore", divide="ignore"):
                wn[s, k] = np.where(t > 0, wt[s, k].astype(np.float64) / t, 0.0).astype(np.float32)
    return wn


def gather(line, offsets, w):
    """win [n * K, C, h, w] of line [n, C, h, Wl]; offsets [n, K]."""
    line = np.asarray(line)
    o = np.asarray(offsets, dtype=np.int64)
    n, K = o.shape
    win = np.empty((n * K,) + line.shape[1:3] + (w,), dtype=line.dtype)
    for s in range(n):
        for k in range(K):
            win[s * K + k] = line[s, :, :, o[s, k]:o[s, k] + w]
    return win


def blend(win, wn, offsets, width, dtype=np.float32):
    """line [n, C, h, width] of win [n * K, C, h, w]; wn [n, K, w], offsets [n, K].  ``dtype=np.float64``: the same sum in float64."""
    win = np.asarray(win, dtype=dtype)
    wn = np.asarray(wn, dtype=np.float32)
    o = np.asarray(offsets, dtype=np.int64)
    n, K = o.shape
    w = win.shape[-1]
    line = np.zeros((n,) + win.shape[1:3] + (width,), dtype=dtype)
    with np.errstate(invalid="ignore"):
        for s in range(n):
            for J in range(width):
                first = True
                for k in range(K):
                    j = J - o[s, k]
                    if j < 0 or j >= w or wn[s, k, j] == 0:
                        continue
                    term = (dtype(wn[s, k, j]) * win[s * K + k, :, :, j]).astype(dtype)
                    line[s, :, :, J] = term if first else (line[s, :, :, J] + term).astype(dtype)
                    first = False
    return line
