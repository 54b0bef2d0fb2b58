"""The device noise stream, restated in plain numpy from its specification ("The noise stream") and from
nothing in the library: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC 2011) and
the Box-Muller transform of its four words.

    counter = (e4, tag, sample & 0xffffffff, sample >> 32)        key = (seed & 0xffffffff, seed >> 32)

``e4`` is the index of a group of four consecutive elements inside one sample, ``sample`` the global row
(``sample_offset + b``), ``tag`` the timestep ``t`` for the step kernels and ``0x80000000 | stream_id`` for ``wd_randn`` and the
posterior kernels.  The uniforms and the angle are fp32 values that the kernel forms exactly as written here (every one of them
is exact, or a single fp32 product); logarithm, square root, sine and cosine are evaluated in float64, so the result is the
value a device draw may differ from by the error of its fp32 ``logf`` / ``sqrtf`` / ``sincosf`` only."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57   # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85   # key bumps (golden ratio, sqrt(3) - 1)
MASK = np.uint64(0xFFFFFFFF)
STREAM = 0x80000000               # tag of wd_randn stream ``id`` is STREAM | id
TWO_PI_F32 = np.float32(6.283185307179586)


def _u64(v):
    if isinstance(v, (int, np.integer)):
        return np.uint64(int(v))
    return np.asarray(v).astype(np.uint64)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds over uint64 arrays that hold 32-bit words (broadcast against each other); returns the four output words."""
    c0, c1, c2, c3, k0, k1 = (_u64(v) & MASK for v in (c0, c1, c2, c3, k0, k1))
    m0, m1 = np.uint64(M0), np.uint64(M1)
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = m0 * c0  # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = m1 * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & MASK, (p0 >> s32) ^ c3 ^ k1, p0 & MASK
        k0 = (k0 + np.uint64(W0)) & MASK
        k1 = (k1 + np.uint64(W1)) & MASK
    return c0, c1, c2, c3


def counter_words(seed, sample, tag, e4):
    """The four Philox output words of one draw (the tail fixtures are conditions on them)."""
    seed, sample = _u64(seed), _u64(sample)
    s32 = np.uint64(32)
    return philox4x32_10(e4, tag, sample & MASK, sample >> s32, seed & MASK, seed >> s32)


def normal4(seed, sample, tag, e4):
    """(z, r): z float64 [..., 4] = (r0 cos a0, r0 sin a0, r1 cos a1, r1 sin a1) and r float64 [..., 4] = (r0, r0, r1, r1), the
    radius each z carries (the tolerance of a device draw is relative to it)."""
    c0, c1, c2, c3 = counter_words(seed, sample, tag, e4)
    s8 = np.uint64(8)
    scale = np.float32(2.0 ** -24)
    one = np.float32(1.0)
    # (0, 1] for the radius, [0, 1) for the angle: 24-bit integers (and 2^24 itself) are exact in fp32, so is the scaling
    u0 = ((c0 >> s8).astype(np.float32) + one) * scale
    u1 = (c1 >> s8).astype(np.float32) * scale
    u2 = ((c2 >> s8).astype(np.float32) + one) * scale
    u3 = (c3 >> s8).astype(np.float32) * scale
    assert u0.dtype == u1.dtype == np.float32
    a0 = (TWO_PI_F32 * u1).astype(np.float32).astype(np.float64)  # the kernel's single fp32 product
    a1 = (TWO_PI_F32 * u3).astype(np.float32).astype(np.float64)
    r0 = np.sqrt(-2.0 * np.log(u0.astype(np.float64)))
    r1 = np.sqrt(-2.0 * np.log(u2.astype(np.float64)))
    z = np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], axis=-1)
    r = np.stack([r0, r0, r1, r1], axis=-1)
    return z, r


def randn(batch, n_per_sample, seed, sample_offset, tag, with_r=False):
    """float64 [batch, n_per_sample]: row b is sample ``sample_offset + b``, elements 4 e4 .. 4 e4 + 3 are draw e4.
    with_r: also the radius of every element, same shape."""
    assert n_per_sample % 4 == 0
    sample = (np.uint64(int(sample_offset)) + np.arange(batch, dtype=np.uint64))[:, None]
    e4 = np.arange(n_per_sample // 4, dtype=np.uint64)[None, :]
    z, r = normal4(seed, sample, tag, e4)
    z, r = z.reshape(batch, n_per_sample), r.reshape(batch, n_per_sample)
    return (z, r) if with_r else z
