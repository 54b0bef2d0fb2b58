"""The host restatement of the noise stream (tests/_philox_ref.py) against what is known independently of this project: the
known-answer vectors of Random123 for philox4x32-10, four counters whose draws sit on the edges of the uniform convention, and
the moments of a standard normal.  No GPU: tests/test_gpu_noise.py holds the device stream to this restatement."""
import math

import numpy as np
import pytest

from tests import _philox_ref as P

# Random123 (kat_vectors, philox4x32 10): counter, key, expected output
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]

# seed 1234, stream 0, e4 = 0: samples whose radius uniform is the smallest (u = 2^-24) or the largest (u = 1) value, found once by
# a scan of samples 0 .. 2^27.  (sample, output word, its top 24 bits, lanes of the draw it governs)
TAIL_SEED = 1234
TAILS = [
    (13898544, 0, 0x000000, (0, 1)),
    (3896489, 0, 0xFFFFFF, (0, 1)),
    (42670038, 2, 0x000000, (2, 3)),
    (4356836, 2, 0xFFFFFF, (2, 3)),
]
R_MAX = math.sqrt(48.0 * math.log(2.0))  # sqrt(-2 ln 2^-24) = 5.768...


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox4x32_10_known_answers(ctr, key, want):
    got = P.philox4x32_10(*ctr, *key)
    assert tuple(int(v) for v in got) == want, [hex(int(v)) for v in got]


def test_philox4x32_10_is_vectorised():
    """All three vectors in one call: what the array form computes per element is what the scalar form computes."""
    cols = [np.array([k[0][i] for k in KAT], dtype=np.uint64) for i in range(4)]
    keys = [np.array([k[1][i] for k in KAT], dtype=np.uint64) for i in range(2)]
    got = P.philox4x32_10(*cols, *keys)
    for i in range(4):
        assert [int(v) for v in got[i]] == [k[2][i] for k in KAT]


@pytest.mark.parametrize("sample,word,top24,lanes", TAILS)
def test_tail_fixtures_exist(sample, word, top24, lanes):
    words = P.counter_words(TAIL_SEED, sample, P.STREAM | 0, 0)
    assert int(words[word]) >> 8 == top24, hex(int(words[word]))
    z, r = P.normal4(TAIL_SEED, sample, P.STREAM | 0, 0)
    assert z.shape == r.shape == (4,) and np.isfinite(z).all()
    if top24 == 0:  # u = 2^-24: the largest radius the stream can produce
        assert abs(r[lanes[0]] - R_MAX) < 1e-12 and r[lanes[0]] == r[lanes[1]]
        assert abs(math.hypot(z[lanes[0]], z[lanes[1]]) - R_MAX) < 1e-12
    else:           # u = 1: radius exactly 0, and the log was of 1, not of 0
        assert r[lanes[0]] == 0.0 and z[lanes[0]] == 0.0 and z[lanes[1]] == 0.0
    assert float(np.abs(z).max()) <= R_MAX + 1e-12


def test_counter_and_key_layout():
    """normal4 / randn place their arguments where the specification says: (e4, tag, sample lo, sample hi), (seed lo, seed hi)."""
    seed, sample, tag, e4 = (5 << 32) | 7, (9 << 32) | 11, 0x80000002, 13
    want = P.philox4x32_10(e4, tag, 11, 9, 7, 5)
    got = P.counter_words(seed, sample, tag, e4)
    assert [int(v) for v in got] == [int(v) for v in want]
    # randn: row b is sample offset + b (with the carry into the high word), element 4 e4 + j is lane j of draw e4
    off = 2 ** 32 - 2
    z = P.randn(4, 12, seed, off, tag)
    assert z.shape == (4, 12)
    for b in range(4):
        for e in range(3):
            one, _ = P.normal4(seed, off + b, tag, e)
            assert np.array_equal(z[b, 4 * e:4 * e + 4], one)
    assert (off + 2) >> 32 == 1  # rows 2 and 3 have a high word
    zr, r = P.randn(4, 12, seed, off, tag, with_r=True)
    assert np.array_equal(zr, z) and r.shape == z.shape and np.array_equal(r[:, 0::4], r[:, 1::4])


def test_reference_moments():
    """2^20 draws of the restated Box-Muller: mean, variance and fourth moment within five standard errors of their estimators
    (Var z = 1, Var z^2 = 2, Var z^4 = E z^8 - 9 = 96)."""
    n = 1 << 20
    z = P.randn(4, n // 4, 1234, 0, P.STREAM | 0).ravel()
    assert z.size == n and np.isfinite(z).all()
    mean, var, m4 = float(z.mean()), float(z.var()), float((z ** 4).mean())
    print(f"reference moments over 2^20 draws: mean {mean:+.2e} var-1 {var - 1:+.2e} m4-3 {m4 - 3:+.2e}")
    assert abs(mean) < 5 / math.sqrt(n)
    assert abs(var - 1) < 5 * math.sqrt(2 / n)
    assert abs(m4 - 3) < 5 * math.sqrt(96 / n)
    # the four lanes of a draw are four different normals, not copies or negations of one another
    q = z.reshape(-1, 4)
    c = np.corrcoef(q.T)
    assert float(np.abs(c - np.eye(4)).max()) < 5 / math.sqrt(n / 4)
