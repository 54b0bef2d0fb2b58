"""wd_xattn_maps (csrc/wd_xattn.hip: xattn_maps_kernel) through the C-ABI, behind guard bands (tests/_guard.py).

x is a window (ld = c + 8, column 4) of a NaN-filled buffer, maps a window (maps_ld = L + 6, column 3) of another; the operands
are the planes wd_xattn_fold writes.  Both forms: the tapped attention alone (mq_pl_a == NULL) and behind a first attention that
runs in full.  (c, heads, L) takes the two widths of the kernel and a key count that is not 10 (the run-time softmax); hw takes one
tile, a ragged last tile of 8 rows (40) and four tiles; batch 3 gives per-sample operand offsets.

Overwrite: against the float64 specification (tests/_xmap_ref.py xattn_maps_spec, scores from the fp32 folded matrix), max-norm
relative 2e-5 - the bound test_gpu_xattn_guard.py holds wd_xattn_fused / wd_xattn_pair to, whose intermediate these
probabilities are.  Accumulate: bit for bit the fp32 replay acc + w * m of the overwrite results.

Largest max_rel against the specification seen on an MI355X (tolerance 2e-5): 3.0e-6 without, 3.8e-6 with the first attention;
on the one-key-dominates inputs the maps equal the specification to 1e-38."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _attn_ref as R  # noqa: E402
from tests import _guard as G  # noqa: E402
from tests import _xmap_ref as X  # noqa: E402
from worddiffusion_amd import _native as N  # noqa: E402

DEV = "cuda:0"
TOL = 2e-5
XHJ = 64


def _st():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


@functools.lru_cache(maxsize=None)
def _layer(B, hw, c, heads, L, seed, step=0, period=1):
    """Operands of one folded cross-attention, folded on the device: (host operands, device dict).  Shared, never modified."""
    lib = N.lib()
    o = R.xattn_operands(B, hw, c, heads, L, seed=seed, step=step, period=period)
    d = c // heads
    dev = {n: o[n].contiguous().to(DEV) for n in ("k", "v", "wq", "wo", "bo", "ga", "be")}
    dev["mq"] = torch.empty(B, heads * L, c, device=DEV)
    dev["mo"] = torch.empty(B, heads * L, c, device=DEV)
    dev["mq_pl"] = torch.zeros(B, 2, XHJ * c, dtype=torch.bfloat16, device=DEV)
    dev["mot_pl"] = torch.zeros(B, 2, XHJ * c, dtype=torch.bfloat16, device=DEV)
    N.check(lib.wd_xattn_fold(dev["k"].data_ptr(), c, dev["v"].data_ptr(), c, B, heads, L, d, float(d ** -0.5), dev["wq"].data_ptr(),
                              dev["wo"].data_ptr(), c, dev["mq"].data_ptr(), dev["mo"].data_ptr(), dev["mq_pl"].data_ptr(),
                              dev["mot_pl"].data_ptr(), _st()), "wd_xattn_fold")
    torch.cuda.synchronize()
    return o, dev


def _spec(x, B, hw, heads, L, la, lb):
    first = None
    if la is not None:
        oa, da = la
        first = (oa["ga"], oa["be"], da["mq"].cpu(), da["mo"].cpu(), oa["bo"])
    ob, db = lb
    return X.xattn_maps_spec(x, B, hw, heads, L, ob["ga"], ob["be"], db["mq"].cpu(), first)


def launch(x, B, hw, c, heads, L, la, lb, mbuf, mview, wtab=None, k_dev=None):
    """One wd_xattn_maps launch on a guarded copy of x into the maps window (mbuf, mview); the guards of both are checked."""
    lib = N.lib()
    xbuf, xv = G.pitched(x, c + 8, 4, 2, DEV)
    a = (None,) * 5 if la is None else tuple(la[1][n].data_ptr() for n in ("ga", "be", "mq_pl", "mot_pl", "bo"))
    b = tuple(lb[1][n].data_ptr() for n in ("ga", "be", "mq_pl"))
    N.check(lib.wd_xattn_maps(xv.data_ptr(), xbuf.shape[-1], B, hw, c, 1e-5, heads, L, *a, *b, mview.data_ptr(), mbuf.shape[-1],
                              None if wtab is None else wtab.data_ptr(), 0 if wtab is None else wtab.numel(),
                              None if k_dev is None else k_dev.data_ptr(), _st()), "wd_xattn_maps")
    torch.cuda.synchronize()
    what = f"(c={c}, heads={heads}, L={L}, hw={hw}, B={B}, {'pair' if la is not None else 'single'})"
    G.assert_untouched(xbuf, xv, "x " + what)
    G.assert_untouched(mbuf, mview, "maps " + what)
    G.assert_finite(mview, "maps " + what)
    return mview.cpu()


def maps_window(B, hw, L):
    return G.guarded(B * hw, L, L + 6, 3, torch.float32, 2, DEV)


@pytest.mark.parametrize("pair", [False, True], ids=["single", "pair"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hw", [16, 40, 64])
@pytest.mark.parametrize("c,heads,L", [(320, 4, 10), (64, 4, 10), (320, 4, 7)])
def test_overwrite_matches_the_float64_specification(c, heads, L, hw, B, pair):
    assert N.lib().wd_xattn_supported(c, heads, L) == 1
    la = _layer(B, hw, c, heads, L, 0) if pair else None
    lb = _layer(B, hw, c, heads, L, 1)
    x = _layer(B, hw, c, heads, L, 0)[0]["x"]
    got = launch(x, B, hw, c, heads, L, la, lb, *maps_window(B, hw, L))
    want = _spec(x, B, hw, heads, L, la, lb)
    e = R.max_rel(got, want)
    print(f"ERR xattn_maps_kernel {'pair' if pair else 'single'} (c={c}, heads={heads}, L={L}, hw={hw}, B={B}): {e:.2e}")
    assert e < TOL
    assert float((got.double().sum(-1) - heads).abs().max()) < 1e-5
    # the dense launch (no pitch, no offset) gives the same bits
    dense = torch.full((B * hw, L), float("nan"), device=DEV)
    lib = N.lib()
    xd = x.to(DEV)
    a = (None,) * 5 if la is None else tuple(la[1][n].data_ptr() for n in ("ga", "be", "mq_pl", "mot_pl", "bo"))
    N.check(lib.wd_xattn_maps(xd.data_ptr(), c, B, hw, c, 1e-5, heads, L, *a, lb[1]["ga"].data_ptr(), lb[1]["be"].data_ptr(),
                              lb[1]["mq_pl"].data_ptr(), dense.data_ptr(), L, None, 0, None, _st()), "wd_xattn_maps")
    assert torch.equal(dense.cpu(), got)


@pytest.mark.parametrize("pair", [False, True], ids=["single", "pair"])
@pytest.mark.parametrize("c,heads,L,hw,B", [(320, 4, 10, 40, 3), (64, 4, 10, 40, 1), (320, 4, 7, 64, 3)])
def test_accumulate_is_the_fp32_replay_of_the_overwrite_results(c, heads, L, hw, B, pair):
    la = _layer(B, hw, c, heads, L, 0) if pair else None
    lb = _layer(B, hw, c, heads, L, 1)
    x0 = _layer(B, hw, c, heads, L, 0)[0]["x"]
    xs = [x0, x0.roll(5, 0).contiguous(), (x0.flip(1) * 0.7 + 0.2).contiguous()]
    ms = [launch(x, B, hw, c, heads, L, la, lb, *maps_window(B, hw, L)).numpy() for x in xs]
    assert not np.array_equal(ms[0], ms[1]) and not np.array_equal(ms[0], ms[2])
    wt = np.array([0.3, 0.0, 1.0 / 3.0], dtype=np.float32)
    wtab = torch.from_numpy(wt).to(DEV)
    k_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    mbuf, mview = maps_window(B, hw, L)
    start = (torch.arange(B * hw * L, dtype=torch.float32).reshape(B * hw, L) % 7) * 0.125
    mview.copy_(start)
    acc = start.numpy()
    for k in range(3):
        k_dev.fill_(k)
        got = launch(xs[k], B, hw, c, heads, L, la, lb, mbuf, mview, wtab, k_dev).numpy()
        want = X.accumulate_fp32(acc, wt[k], ms[k])
        if k == 1:
            assert np.array_equal(want, acc)  # a weight of 0 switches the step off
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), f"step {k}: not acc + w * m with two roundings"
        acc = want
    # (the fused form would differ: the two-rounding replay is not the fma)
    fma = (start.numpy().astype(np.float64) + np.float64(wt[0]) * ms[0].astype(np.float64)).astype(np.float32)
    assert not np.array_equal(fma, X.accumulate_fp32(start.numpy(), wt[0], ms[0]))
    k_dev.fill_(3)  # an index outside the table adds nothing
    assert np.array_equal(launch(xs[0], B, hw, c, heads, L, la, lb, mbuf, mview, wtab, k_dev).numpy(), acc)


@pytest.mark.parametrize("pair", [False, True], ids=["single", "pair"])
@pytest.mark.parametrize("B,hw,c,heads,L", [(2, 40, 320, 4, 10), (2, 33, 64, 4, 10)])
def test_one_key_dominating_by_80_does_not_overflow(B, hw, c, heads, L, pair):
    """The staircase of tests/_attn_ref.py xattn_operands with one stair: step 80, period L - 1, so the last key's logit is 80
    above the level of all the others (exp(80) overflows nothing only if the maximum is subtracted first)."""
    la = _layer(B, hw, c, heads, L, 0) if pair else None
    lb = _layer(B, hw, c, heads, L, 1, 80, L - 1)
    x = _layer(B, hw, c, heads, L, 0)[0]["x"]
    got = launch(x, B, hw, c, heads, L, la, lb, *maps_window(B, hw, L))
    want = _spec(x, B, hw, heads, L, la, lb)
    assert float(want[:, L - 1].min()) > heads - 1e-6  # the specification itself: all the mass on the last key
    e = R.max_rel(got, want)
    print(f"ERR xattn_maps_kernel staircase {'pair' if pair else 'single'} (c={c}, hw={hw}): {e:.2e}")
    assert e < TOL
    assert float((got.double().sum(-1) - heads).abs().max()) < 1e-5


def test_bad_arguments_are_refused_without_a_launch():
    lib = N.lib()
    B, hw, c, heads, L = 1, 16, 320, 4, 10
    z = torch.zeros(B * hw * 64, device=DEV)
    zb = torch.zeros(2 * XHJ * c, dtype=torch.bfloat16, device=DEV)
    ki = torch.zeros(1, dtype=torch.int32, device=DEV)
    p, pb = z.data_ptr(), zb.data_ptr()

    def call(heads=heads, L=L, maps=p, wtab=None, wtab_n=0, k_dev=None, ld=c, c=c, a=(None,) * 5):
        return lib.wd_xattn_maps(p, ld, B, hw, c, 1e-5, heads, L, *a, p, p, pb, maps, L, wtab, wtab_n, k_dev, _st())

    assert call(L=11) == N.WD_EINVAL            # heads * L = 44 > 40
    assert call(heads=5, L=10) == N.WD_EINVAL
    assert call(c=128) == N.WD_EINVAL
    assert call(maps=None) == N.WD_EINVAL
    assert call(wtab=p, wtab_n=4) == N.WD_EINVAL  # wtab without k_dev
    assert call(k_dev=ki.data_ptr()) == N.WD_EINVAL
    assert call(wtab=p, wtab_n=0, k_dev=ki.data_ptr()) == N.WD_EINVAL
    assert call(ld=c + 2) == N.WD_EINVAL
    assert call(a=(p, p, pb, None, p)) == N.WD_EINVAL  # a first attention without its Mo planes
    torch.cuda.synchronize()
    assert not bool(z.any()) and not bool(zb.any())
