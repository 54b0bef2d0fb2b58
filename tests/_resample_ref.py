"""Resampling jumps of a known-region call (RePaint, Lugmayr et al. 2022, section 4.2 and algorithm 1), restated in numpy and
float64 from their specification (DESIGN.md "Resampling jumps") and from nothing in the library.  A test helper (not collected).

The walk over the levels ``tau[0..S-1]`` the plain call would visit, ``land(i) = tau[i + 1]`` (0 after the last entry):

    m = 0
    while m < S:
        down(m); m += 1
        if m % j == 0 and m < S:
            repeat r - 1 times:   up from level tau[m] to level tau[m - j];   down(m - j) .. down(m - 1)

Entry k of the walk starts from the level ``tau'[k]``.  A down entry carries its sampler's own five coefficients, computed from
(level from, level to); an up entry carries g1 = fp32(sqrt(Q/A)), g2 = fp32(sqrt(1 - Q/A)) with A = alpha_hat[from],
Q = alpha_hat[to], and is  x = g1 * x + g2 * z  in fp32, both products and the sum rounded on their own.

Draws come from the device noise stream (``tests/_philox_ref.py``) under a fourth tag family,

    tag = TAG_WALK | which << 26 | k        TAG_WALK = 0xC0000000,  k < 2^26 the WALK INDEX,
    which = 0: a down entry's step noise,  1: its blend noise,  2: an up entry's jump noise,

so every visit of a level draws afresh.  The other three families: a bare timestep t < 2^30 (the step kernels of a plain call),
``0x40000000 | p`` (the blend of a plain call at level p < 2^30) and ``0x80000000 | stream_id`` (``wd_randn``, ids < 2^30)."""
import math

import numpy as np

from tests import _philox_ref as P

TAG_WALK = 0xC0000000
TAG_KNOWN = 0x40000000
STEP, BLEND, JUMP = 0, 1, 2
K_BOUND, T_BOUND = 2 ** 26, 2 ** 30


def walk(tau, j, r):
    """[(kind, level from, level to, m)]: kind "down" with m the index into ``tau``, or "up" with m None."""
    tau = [int(t) for t in tau]
    S = len(tau)
    out = []

    def down(i):
        out.append(("down", tau[i], tau[i + 1] if i + 1 < S else 0, i))
    m = 0
    while m < S:
        down(m)
        m += 1
        if m % j == 0 and m < S:
            for _ in range(r - 1):
                out.append(("up", tau[m], tau[m - j], None))
                for i in range(m - j, m):
                    down(i)
    return out


def counts(S, j, r):
    """(down entries, up entries) of the walk."""
    jumps = (r - 1) * ((S - 1) // j)
    return S + jumps * j, jumps


def alpha_hat64(noise_steps=1000):
    """alpha_hat of the reference's schedule, float64 numpy (``tests/_ddim_ref.py``: the fp32 betas, everything after in float64)."""
    from tests._ddim_ref import alpha_hat64 as ah
    return ah(noise_steps).numpy()


def jump_tables(entries, ah):
    """(g1, g2) fp32 [entries]: the jump's coefficients at the up entries, 0 at the down entries."""
    g1 = np.zeros(len(entries), dtype=np.float32)
    g2 = np.zeros(len(entries), dtype=np.float32)
    for k, (kind, frm, to, _) in enumerate(entries):
        if kind == "up":
            ratio = float(ah[to]) / float(ah[frm])
            g1[k] = np.float32(math.sqrt(ratio))
            g2[k] = np.float32(math.sqrt(1.0 - ratio))
    return g1, g2


def ddim_tables(entries, ah, eta):
    """float64 [5, entries]: c1 = sqrt(1-a), c2 = 1/sqrt(a), c3 = sqrt(p), c4 = sqrt(max(1-p-sigma^2, 0)), c5 = sigma with
    a = alpha_hat[from], p = alpha_hat[to], sigma = eta sqrt((1-p)/(1-a)) sqrt(1 - a/p), at the down entries; 0 at the up entries."""
    c = np.zeros((5, len(entries)))
    for k, (kind, frm, to, _) in enumerate(entries):
        if kind == "down":
            a, p = float(ah[frm]), float(ah[to])
            sigma = eta * math.sqrt((1 - p) / (1 - a)) * math.sqrt(1 - a / p)
            c[:, k] = [math.sqrt(1 - a), 1 / math.sqrt(a), math.sqrt(p), math.sqrt(max(1 - p - sigma * sigma, 0.0)), sigma]
    return c


def dpmpp_tables(entries, ah, order=2):
    """float64 [5, entries]: c1 = sqrt(1-a), c2 = 1/sqrt(a), c3 = sqrt((1-p)/(1-a)), c4 = -sqrt(p) expm1(-h), c5 = h / (2 h_prev)
    with h = lambda(p) - lambda(a), lambda(v) = ln(v / (1-v)) / 2 and h_prev the h of the preceding down entry of the walk.
    c5 = 0 (first order): the first entry, the entry that lands on level 0, every entry at order 1, and the first down entry
    after an up entry."""
    lam = lambda v: 0.5 * math.log(v / (1 - v))  # noqa: E731
    c = np.zeros((5, len(entries)))
    h_prev, after_up = None, False
    for k, (kind, frm, to, _) in enumerate(entries):
        if kind == "up":
            after_up = True
            continue
        a, p = float(ah[frm]), float(ah[to])
        h = lam(p) - lam(a)
        first_order = order == 1 or h_prev is None or after_up or to == 0
        c[:, k] = [math.sqrt(1 - a), 1 / math.sqrt(a), math.sqrt((1 - p) / (1 - a)), -math.sqrt(p) * math.expm1(-h),
                   0.0 if first_order else h / (2 * h_prev)]
        h_prev, after_up = h, False
    return c


def forward_jump(x, g1, g2, z):
    """x after an up entry, fp32: numpy rounds each fp32 operation once, nothing is fused."""
    x, z = np.asarray(x, dtype=np.float32), np.asarray(z, dtype=np.float32)
    g1, g2 = np.float32(g1), np.float32(g2)
    return ((g1 * x).astype(np.float32) + (g2 * z).astype(np.float32)).astype(np.float32)


def forward_jump64(x, ah, frm, to, z):
    """The same in float64, from the levels."""
    ratio = float(ah[to]) / float(ah[frm])
    return math.sqrt(ratio) * x + math.sqrt(1.0 - ratio) * z


def tag(which, k):
    assert which in (STEP, BLEND, JUMP) and 0 <= k < K_BOUND
    return TAG_WALK | (which << 26) | int(k)


def draw(batch, n_per_sample, seed, sample_offset, which, k, with_r=False):
    """What draw ``which`` of walk entry k is for rows sample_offset .. + batch: float64 [batch, n_per_sample] (and the radii)."""
    return P.randn(batch, n_per_sample, seed, sample_offset, tag(which, k), with_r=with_r)


def family(t):
    """Which of the four tag families a 32-bit tag belongs to: its top two bits."""
    return (int(t) >> 30) & 3
