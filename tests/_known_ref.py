"""The known-region blend (``wd_known_blend``, include/wdiff_hip.h), restated in numpy fp32 from its specification and from
nothing in the library.  A test helper (not collected).

After a sampler's update and before its timestep advance, x is at the level of the predecessor p of the step just taken:

    DDPM form (no table):   p = t - 1
    table form:             p = tau[k + 1] if k + 1 < S else 0

and per element, every operation rounded to fp32 on its own (numpy rounds each fp32 operation once: nothing is fused),

    kv = x0                                   if p == 0   (the trajectory ends on the known latent itself)
    kv = sqrt_ah[p] * x0 + sqrt_1m_ah[p] * z  otherwise   (the expression of noise_images)
    x  = x  where m == 0,   kv  where m == 1,   x + m * (kv - x)  otherwise.

z is the caller's, or drawn from the device noise stream (``tests/_philox_ref.py``) with

    counter = (e4, tag, sample & 0xffffffff, sample >> 32)        key = (seed & 0xffffffff, seed >> 32)

whose ``tag`` is now one of three disjoint families: the timestep ``t`` (< 2^30) for the step kernels, ``0x80000000 | stream_id``
for ``wd_randn`` and the posterior kernels (stream 4, ``STREAM_KNOWN``: the per-sample fixed eps of a known-region call), and
``0x40000000 | p`` (``TAG_KNOWN | p``) for the blend at level p.  The draw of a group of four does not depend on the mask."""
import numpy as np

from tests import _philox_ref as P

TAG_KNOWN = 0x40000000  # tag of the blend's draw at level p is TAG_KNOWN | p
STREAM_KNOWN = 4        # wd_randn stream of the fixed eps (tag P.STREAM | 4)


def predecessor(t=None, k=None, tau=None):
    """The level x is at when the blend runs: ``t - 1`` (DDPM form, ``tau`` None) or the entry after ``tau[k]`` (0 after the last)."""
    if tau is None:
        return max(int(t) - 1, 0)
    return int(tau[k + 1]) if k + 1 < len(tau) else 0


def draw(batch, n_per_sample, seed, sample_offset, p, with_r=False):
    """What the blend draws at level p for rows sample_offset .. + batch: float64 [batch, n_per_sample] (and the radii)."""
    return P.randn(batch, n_per_sample, seed, sample_offset, TAG_KNOWN | int(p), with_r=with_r)


def fixed_eps(batch, n_per_sample, seed, sample_offset, with_r=False):
    """The per-sample fixed eps of a call: stream STREAM_KNOWN of ``wd_randn``."""
    return P.randn(batch, n_per_sample, seed, sample_offset, P.STREAM | STREAM_KNOWN, with_r=with_r)


def known_value(x0, p, sqrt_ah, sqrt_1m_ah, z):
    """kv: the known latent at level p, fp32."""
    x0 = np.asarray(x0, dtype=np.float32)
    if p == 0:
        return x0.copy()
    sa, sb = np.float32(sqrt_ah[p]), np.float32(sqrt_1m_ah[p])
    z = np.asarray(z, dtype=np.float32)
    return ((sa * x0).astype(np.float32) + (sb * z).astype(np.float32)).astype(np.float32)


def blend(x, x0, mask, p, sqrt_ah, sqrt_1m_ah, z=None):
    """x after the blend at level p; all operands fp32 arrays of one shape (z may be None at p == 0: it is not read)."""
    x = np.asarray(x, dtype=np.float32)
    m = np.asarray(mask, dtype=np.float32)
    kv = known_value(x0, p, sqrt_ah, sqrt_1m_ah, z)
    with np.errstate(invalid="ignore"):
        mixed = (x + (m * (kv - x).astype(np.float32)).astype(np.float32)).astype(np.float32)
    return np.where(m == 0, x, np.where(m == 1, kv, mixed)).astype(np.float32)


def retained(tau, start):
    """The visited timesteps a call with ``start`` keeps of its usual schedule ``tau``; the first is the level noised to."""
    return [int(t) for t in tau if t <= start]
