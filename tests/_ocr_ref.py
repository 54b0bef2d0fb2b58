"""Float64 specification of the CTC loss of OCR-aware training (``wd_ctc_loss``, include/wdiff_hip.h): log-softmax + CTC with
the blank at class 0, ``reduction='sum'``, ``zero_infinity`` on, and the gradient with respect to the RAW logits.

It is written in the log domain, step by step over the blank-extended target, and is therefore independent of the kernel's
formulation (a scaled linear-domain recursion): tests/test_ocr_ref_host.py holds it to ``torch.nn.functional.ctc_loss`` in float64
on ``CASES``.  The case table is shared by the host test and tests/test_gpu_ctc.py.  numpy only."""
import functools

import numpy as np

NEG = -np.inf


def _lse(*xs):
    m = functools.reduce(np.maximum, xs)
    safe = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return np.where(np.isfinite(m), safe + np.log(sum(np.exp(x - safe) for x in xs)), NEG)


def check_sample(C, T, Lmax, ids, input_len, target_len) -> int:
    """The status word of one sample: bit 0 input_len outside [1, T], bit 1 target_len outside [0, Lmax], bit 2 an id (of the
    first target_len ones) outside [0, C)."""
    st = 0
    if not 1 <= input_len <= T:
        st |= 1
    if not 0 <= target_len <= Lmax:
        st |= 2
    elif any(not 0 <= int(i) < C for i in ids[:target_len]):
        st |= 4
    return st


def ctc_sample(x, ids):
    """One sample: x float64 [T', C] raw logits over the steps that count, ids the target (any length >= 0) ->
    (nll, gamma [T', C]): gamma[t, c] = sum over the states that carry class c of their posterior at t (zeros when nll = inf)."""
    Tn, C = x.shape
    m = x.max(1, keepdims=True)
    lp = x - (m + np.log(np.exp(x - m).sum(1, keepdims=True)))  # log-softmax
    ext = [0]
    for i in ids:
        ext += [int(i), 0]
    ext = np.array(ext)
    S = len(ext)
    skip = np.zeros(S, bool)
    skip[2:] = ext[2:] != ext[:-2]
    la = np.full((Tn, S), NEG)
    la[0, 0] = lp[0, 0]
    if S > 1:
        la[0, 1] = lp[0, ext[1]]
    for t in range(1, Tn):
        pad = np.concatenate([[NEG, NEG], la[t - 1]])
        p1, p2 = pad[1:S + 1], np.where(skip, pad[:S], NEG)
        la[t] = _lse(la[t - 1], p1, p2) + lp[t, ext]
    lb = np.full((Tn, S), NEG)  # beta including its own emission (torch's convention)
    lb[Tn - 1, S - 1] = lp[Tn - 1, 0]
    if S > 1:
        lb[Tn - 1, S - 2] = lp[Tn - 1, ext[S - 2]]
    skipf = np.zeros(S, bool)
    skipf[:-2] = ext[2:] != ext[:-2]
    for t in range(Tn - 2, -1, -1):
        pad = np.concatenate([lb[t + 1], [NEG, NEG]])
        n1, n2 = pad[1:S + 1], np.where(skipf, pad[2:S + 2], NEG)
        lb[t] = _lse(lb[t + 1], n1, n2) + lp[t, ext]
    ll = float(_lse(la[Tn - 1, S - 1], la[Tn - 1, S - 2] if S > 1 else np.float64(NEG)))
    gamma = np.zeros((Tn, C))
    if not np.isfinite(ll):
        return np.inf, gamma
    with np.errstate(invalid="ignore"):
        post = np.exp(la + lb - lp[:, ext] - ll)  # [T', S]; -inf - -inf cannot occur: lp is finite
    post = np.nan_to_num(post, nan=0.0)
    for s in range(S):
        gamma[:, ext[s]] += post[:, s]
    return -ll, gamma


def ctc_loss(logits, targets, input_len, target_len, scale=1.0):
    """logits [T, B, C] (any float), targets int [B, Lmax] -> dict(loss, sample_nll [B], dlogits [T, B, C], status [B]) in
    float64.  loss = scale * sum of the finite nll of the valid samples; a sample with status != 0 or nll = inf has a zero
    gradient; the sample_nll of an invalid sample is 0, of an infeasible one inf."""
    x = np.asarray(logits, np.float64)
    T, B, C = x.shape
    targets = np.asarray(targets).reshape(B, -1)
    nll, status, g = np.zeros(B), np.zeros(B, np.int32), np.zeros_like(x)
    for b in range(B):
        status[b] = check_sample(C, T, targets.shape[1], targets[b], int(input_len[b]), int(target_len[b]))
        if status[b]:
            continue
        Tn = int(input_len[b])
        xb = x[:Tn, b]
        nll[b], gamma = ctc_sample(xb, targets[b, :int(target_len[b])])
        if np.isfinite(nll[b]):
            m = xb.max(1, keepdims=True)
            p = np.exp(xb - m)
            g[:Tn, b] = scale * (p / p.sum(1, keepdims=True) - gamma)
    return dict(loss=scale * float(nll[np.isfinite(nll) & (status == 0)].sum()), sample_nll=nll, dlogits=g, status=status)


# ---- the case table ----------------------------------------------------------------------------------------------------------
def _case(name, T, B, C, Lmax, seed, logit_scale=1.0, input_len=None, target_len=None, targets=None, lo=1):
    """Random ids in [lo, C) unless given; lengths default to T and Lmax."""
    rs = np.random.RandomState(seed)
    x = (logit_scale * rs.standard_normal((T, B, C))).astype(np.float32)
    if targets is None:
        targets = rs.randint(lo, C, (B, max(Lmax, 1)))
    targets = np.asarray(targets, np.int64).reshape(B, -1)
    il = np.full(B, T, np.int32) if input_len is None else np.asarray(input_len, np.int32)
    tl = np.full(B, Lmax, np.int32) if target_len is None else np.asarray(target_len, np.int32)
    return dict(name=name, logits=x, targets=targets, input_len=il, target_len=tl)


def _build_cases():
    c = []
    c.append(_case("T1_L1", 1, 2, 51, 1, 1))
    c.append(_case("T1_L0", 1, 1, 51, 1, 2, target_len=[0]))
    c.append(_case("T5_L0", 5, 2, 51, 3, 3, target_len=[0, 0]))
    # 'aab' needs a blank between the a's: T = L + repeats = 4 is the shortest feasible, T = 3 is infeasible (inf -> zero)
    c.append(_case("repeat_exact", 4, 2, 51, 3, 4, targets=[[7, 7, 9], [7, 8, 9]]))
    c.append(_case("repeat_one_short", 3, 2, 51, 3, 5, targets=[[7, 7, 9], [7, 8, 9]]))
    c.append(_case("ids_equal_blank", 12, 3, 51, 4, 6, targets=[[0, 3, 0, 0], [0, 0, 0, 0], [5, 0, 5, 1]]))
    c.append(_case("input_len_short", 20, 3, 51, 5, 7, input_len=[20, 11, 6], target_len=[5, 5, 2]))
    c.append(_case("L31", 80, 2, 51, 31, 8))
    c.append(_case("L32", 80, 2, 51, 32, 9))
    c.append(_case("L42", 100, 2, 54, 42, 10))
    c.append(_case("L64", 140, 1, 51, 64, 11))
    c.append(_case("L127_C5", 256, 1, 5, 127, 12))
    c.append(_case("C54", 30, 2, 54, 6, 13, lo=0))
    c.append(_case("C256", 40, 2, 256, 10, 14))
    c.append(_case("C1_blank_only", 6, 1, 1, 2, 15, target_len=[0], targets=[[0, 0]]))
    for sc in (1, 8, 30):
        c.append(_case(f"T256_scale{sc}", 256, 3, 51, 10, 20 + sc, logit_scale=float(sc), input_len=[256, 200, 256],
                       target_len=[10, 7, 10], targets=np.array([[3, 9, 9, 9, 2, 50, 1, 1, 4, 6], [8, 8, 1, 2, 3, 4, 5, 6, 7, 8],
                                                                 [0, 4, 0, 0, 4, 4, 17, 23, 0, 1]])))
    c.append(_case("T1024", 1024, 1, 51, 20, 16, logit_scale=4.0))
    c.append(_case("B1", 33, 1, 51, 7, 17))
    c.append(_case("B5_mixed", 37, 5, 51, 9, 18, input_len=[37, 1, 20, 36, 9], target_len=[9, 1, 0, 3, 9]))
    return c


CASES = _build_cases()
CASE_IDS = [c["name"] for c in CASES]


def grad_error(g, r):
    """(err, bar) of the project's gradient bar for one sample: err = ||g - r||, bar = 2e-4 ||r|| + 1e-7."""
    g, r = np.asarray(g, np.float64), np.asarray(r, np.float64)
    return float(np.linalg.norm(g - r)), 2e-4 * float(np.linalg.norm(r)) + 1e-7


def torch_ctc(case, dtype, scale=1.0):
    """torch's own CTC on the CPU in ``dtype``: (loss, sample_nll [B] as torch reports it, dlogits [T, B, C]).  Samples whose
    lengths or ids torch would reject must not be in ``case``."""
    import torch
    x = torch.tensor(case["logits"], dtype=dtype, requires_grad=True)
    lp = torch.log_softmax(x, 2)
    tg, il, tl = (torch.as_tensor(case[k]).long() for k in ("targets", "input_len", "target_len"))
    nll = torch.nn.functional.ctc_loss(lp, tg, il, tl, blank=0, reduction="none", zero_infinity=True)
    loss = scale * nll.sum()
    loss.backward()
    return float(loss.detach()), nll.detach().double().numpy(), x.grad.double().numpy()


def greedy_decode(logits):
    """argmax per step, collapse repeats, drop blanks -> a list of id lists, one per sample (logits [T, B, C])."""
    best = np.asarray(logits).argmax(2)  # [T, B]
    out = []
    for b in range(best.shape[1]):
        seq, prev = [], -1
        for k in best[:, b]:
            if k != prev and k != 0:
                seq.append(int(k))
            prev = k
        out.append(seq)
    return out
