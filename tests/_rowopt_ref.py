"""numpy fp32 specification of the row-wise kernels (include/wdiff_hip.h: wd_row_slots, wd_adamw_rows).  Every operation is one
fp32 numpy operation, so every intermediate is rounded on its own and nothing is contracted; the scalars are formed in double and
rounded once, as the C entry point forms them."""
import math

import numpy as np

F = np.float32


def row_slots(ids, rows):
    """slots[b] = j where rows[j] == ids[b], else -1 (ids: any int64 values; rows: distinct)."""
    ids = np.asarray(ids, dtype=np.int64)
    out = np.full(ids.shape, -1, dtype=np.int64)
    for j, r in enumerate(rows):
        out[ids == int(r)] = j
    return out


def embedding_bwd(slots, d, nrows):
    """wd_embedding_bwd into a compact [nrows][c] buffer: rows added with r ascending, starting from 0.0f."""
    d = np.asarray(d, dtype=F)
    out = np.zeros((nrows, d.shape[1]), dtype=F)
    for r, s in enumerate(np.asarray(slots)):
        if 0 <= s < nrows:
            out[s] = out[s] + d[r]
    return out


def scalars(lr, beta1, beta2, eps, weight_decay, step):
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    return dict(decay=F(1.0 - lr * weight_decay), lrwd=F(lr * weight_decay), omb1=F(1.0 - beta1), b2=F(beta2), omb2=F(1.0 - beta2),
                step_size=F(lr / bc1), bc2_sqrt=F(math.sqrt(bc2)), eps=F(eps))


def adamw_rows(table, rows, grad, m, v, step, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, anchor=None,
               ema_table=None, ema_mode=0, ema_beta=0.995, gscale=None):
    """One wd_adamw_rows call on copies: (table, m, v, ema_table or None).  table [vocab][c] (the logical table, without pitch),
    grad / m / v / anchor compact [len(rows)][c]."""
    k = scalars(lr, beta1, beta2, eps, weight_decay, step)
    table, m, v = np.array(table, dtype=F), np.array(m, dtype=F), np.array(v, dtype=F)
    ema = None if ema_table is None else np.array(ema_table, dtype=F)
    ema_b, ema_omb = F(ema_beta), F(1.0 - ema_beta)
    with np.errstate(all="ignore"):
        for j, r in enumerate(rows):
            g = np.asarray(grad[j], dtype=F)
            if gscale is not None:
                g = g * F(gscale)
            p = table[r]
            if anchor is not None:
                p = p - k["lrwd"] * (p - np.asarray(anchor[j], dtype=F))
            else:
                p = p * k["decay"]
            mj = m[j] + k["omb1"] * (g - m[j])
            vj = v[j] * k["b2"]
            vj = vj + (k["omb2"] * g) * g
            denom = np.sqrt(vj) / k["bc2_sqrt"] + k["eps"]
            p = p + (-k["step_size"] * mj) / denom
            assert p.dtype == F and mj.dtype == F and vj.dtype == F
            table[r], m[j], v[j] = p, mj, vj
            if ema is not None and ema_mode == 1:
                ema[r] = p
            elif ema is not None and ema_mode == 2:
                ema[r] = ema[r] * ema_b + ema_omb * p
    return table, m, v, ema
