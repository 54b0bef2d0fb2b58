"""The five streaming kernels of the PHOSCnet recogniser (csrc/wd_phoscnet.hip) behind guard bands, against the numpy
specifications of tests/_phoscnet_ref.py (held to torch on the CPU by tests/test_phoscnet_host.py).

Every operand is a window of a wider, taller buffer filled with a NaN pattern (tests/_guard.py): a store outside the window
changes the pattern, a read outside it brings a NaN into the result.

Bit for bit: wd_relu_pool_planes and wd_tpp_max (planes as int16, fp32 with torch.equal) and wd_resize_bilinear.
wd_phosc_finish: the ReLU half exact; the sigmoid within 1e-6 absolute of float64 - its slope is at most 1/4, an expf within a
few ulp and two roundings give <~ 2e-7, 1e-6 leaves a factor 5.
wd_phosc_score: within 1e-4 of float64 - three length-769 fp32 reductions, at most 2 * 769 * 2^-24 ~ 9.2e-5 relative on values
of at most 1; the best index equals the float64 one on inputs whose best-to-second gap exceeds 1e-2 (asserted: a condition the
construction meets, not a tolerance)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _guard as G  # noqa: E402
from tests import _phoscnet_ref as R  # noqa: E402
from worddiffusion_amd import _native as N  # noqa: E402

DEV = "cuda:0"


def _st():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _bits(p):
    return p.detach().cpu().contiguous().view(torch.int16)


def _spec_bits(v):
    hi, lo = R.split_np(v)
    return torch.from_numpy(np.stack([hi, lo]).view(np.int16))


def _map(rs, rows, c):
    """Negatives, +-0, values with a non-zero lo plane (any fp32 with more than 8 significant bits) and exact bf16 values."""
    x = rs.standard_normal((rows, c)).astype(np.float32) * 3.0
    flat = x.reshape(-1)
    flat[::7] = 0.0
    flat[3::11] = -0.0
    flat[5::13] = np.float32(1.5)       # exact in bf16: lo = 0
    flat[6::17] = np.float32(1.0 + 2.0 ** -12)   # hi = 1, lo = 2^-12
    return x


# ---- wd_relu_pool_planes ---------------------------------------------------------------------------------------------------
def _relu_pool(x, batch, h, w, pool, ld_in, col_in, ld_out, col_out, lo=True):
    c = x.shape[1]
    ho, wo = (h // 2, w // 2) if pool == 2 else (h, w)
    xbuf, xv = G.pitched(torch.from_numpy(x), ld_in, col_in, device=DEV)
    obuf, ov = G.guarded(batch * ho * wo, c, ld_out, col_out, torch.bfloat16, device=DEV, planes=2)
    rc = N.lib().wd_relu_pool_planes(xv.data_ptr(), ld_in, batch, h, w, c, pool, ov[0].data_ptr(), ov[1].data_ptr() if lo else None,
                                     ld_out, _st())
    assert rc == N.WD_OK
    torch.cuda.synchronize()
    G.assert_untouched(xbuf, xv, "x")
    want = _spec_bits(R.relu_pool_np(x, batch, h, w, pool))
    if lo:
        G.assert_untouched(obuf, ov, "planes")
        G.assert_finite(ov, "planes")
        assert torch.equal(_bits(ov), want)
    else:
        G.assert_untouched(obuf[0], ov[0], "hi plane")
        assert bool((obuf[1].view(torch.int16) == G.NAN16).all()), "the lo plane was passed nowhere"
        assert torch.equal(_bits(ov[0]), want[0])
    return want


@pytest.mark.parametrize("batch,h,w,c,pool", [(2, 5, 7, 64, 1), (2, 5, 7, 64, 2), (1, 2, 2, 32, 2), (3, 1, 1, 4096, 1)])
def test_relu_pool_planes_bit_for_bit(batch, h, w, c, pool):
    x = _map(np.random.RandomState(1), batch * h * w, c)
    want = _relu_pool(x, batch, h, w, pool, c + 8, 4, c + 16, 8)
    assert bool((want[1] != 0).any()) and bool((want[0] == 0).any())  # lo planes that carry something, ReLU zeros
    _relu_pool(x, batch, h, w, pool, c + 8, 4, c + 16, 8, lo=False)


def test_relu_pool_planes_element_path_on_an_odd_pitch():
    x = _map(np.random.RandomState(2), 2 * 5 * 7, 64)
    for pool in (1, 2):
        _relu_pool(x, 2, 5, 7, pool, 67, 1, 69, 3)     # pitches and columns off the 16-byte grid
    x = _map(np.random.RandomState(3), 2 * 4 * 6, 30)  # a channel count that is no multiple of 4
    _relu_pool(x, 2, 4, 6, 2, 32, 0, 32, 0)


def test_relu_pool_planes_second_grid_pass_begins_inside_the_last_sample():
    # 2048 workgroups x 256 threads x 4 channels cover 32768 rows of 64 channels: sample 2 of 3 x (110 x 100) begins at row 22000
    batch, h, w, c = 3, 110, 100, 64
    assert 22000 < 2048 * 256 // (c // 4) < batch * h * w
    _relu_pool(_map(np.random.RandomState(4), batch * h * w, c), batch, h, w, 1, c, 0, c, 0)
    # pooled: 2 x (363 x 364) -> 2 x (181 x 182) = 65884 output rows, the second pass begins inside sample 1
    batch, h, w, c = 2, 363, 364, 32
    assert (h // 2) * (w // 2) < 2048 * 256 // (c // 4) < batch * (h // 2) * (w // 2)
    _relu_pool(_map(np.random.RandomState(5), batch * h * w, c), batch, h, w, 2, c, 0, c, 0)


def test_relu_pool_planes_refusals():
    lib, p = N.lib(), 4096  # (a refused call returns before any launch: the address is never used)
    bad = [dict(x=None), dict(hi=None), dict(batch=0), dict(h=0), dict(c=0), dict(pool=3), dict(pool=0), dict(pool=2, h=1),
           dict(pool=2, w=1), dict(ld_in=63), dict(ld_out=63)]
    for kw in bad:
        a = dict(x=p, ld_in=64, batch=1, h=2, w=2, c=64, pool=1, hi=p, lo=p, ld_out=64)
        a.update(kw)
        assert lib.wd_relu_pool_planes(a["x"], a["ld_in"], a["batch"], a["h"], a["w"], a["c"], a["pool"], a["hi"], a["lo"], a["ld_out"],
                                       _st()) == N.WD_EINVAL, kw


# ---- wd_tpp_max ------------------------------------------------------------------------------------------------------------
def _tpp(x, batch, h, w, levels=R.LEVELS, ld=None, col=0, f32=True, lo=True):
    c = x.shape[1]
    ncol = c * sum(levels)
    xbuf, xv = G.pitched(torch.from_numpy(x), c if ld is None else ld, col, device=DEV)
    fbuf, fv = G.guarded(batch, ncol, ncol + 12, 4, torch.float32, device=DEV)
    pbuf, pv = G.guarded(batch, ncol, ncol + 8, 8, torch.bfloat16, device=DEV, planes=2)
    lv = (C.c_int32 * len(levels))(*levels)
    rc = N.lib().wd_tpp_max(xv.data_ptr(), xbuf.shape[-1], batch, h, w, c, C.addressof(lv), len(levels), fv.data_ptr() if f32 else None,
                            ncol + 12, pv[0].data_ptr(), pv[1].data_ptr() if lo else None, ncol + 8, _st())
    assert rc == N.WD_OK
    torch.cuda.synchronize()
    want = R.tpp_np(x, batch, h, w, levels)
    G.assert_untouched(xbuf, xv, "x")
    if f32:
        G.assert_untouched(fbuf, fv, "features")
        G.assert_finite(fv, "features")
        assert torch.equal(fv.cpu(), torch.from_numpy(want))
    else:
        assert bool((fbuf.view(torch.int32) == G.NAN32).all()), "out_f32 was passed nowhere"
    if lo:
        G.assert_untouched(pbuf, pv, "planes")
        G.assert_finite(pv, "planes")
        assert torch.equal(_bits(pv), _spec_bits(want))
    else:
        G.assert_untouched(pbuf[0], pv[0], "hi plane")
        assert torch.equal(_bits(pv[0]), _spec_bits(want)[0])
    return want


@pytest.mark.parametrize("h,w,c", [(3, 62, 32), (3, 62, 512), (2, 4, 32), (1, 5, 512)])
def test_tpp_max_bit_for_bit(h, w, c):
    x = _map(np.random.RandomState(6), 2 * h * w, c)
    want = _tpp(x, 2, h, w)
    if w == 4:  # level 5: k = 1, one zero column on the right: bin 4 holds padding only
        assert not want.reshape(2, -1)[:, 3 * c:].reshape(2, c, 5)[:, :, 4].any()
    _tpp(x, 2, h, w, f32=False)
    _tpp(x, 2, h, w, lo=False)


def test_tpp_max_padding_split_and_negative_input():
    # w = 62, level 5: k = 13, 3 zero columns, 1 on the left and 2 on the right - bin 0 is columns 0..11, bin 4 columns 51..61
    x = np.full((3 * 62, 32), -1.0, dtype=np.float32)
    xr = x.reshape(3, 62, 32)
    xr[0, 11, 0], xr[1, 12, 1], xr[2, 50, 2], xr[0, 51, 3] = 2.0, 3.0, 4.0, 5.0
    want = _tpp(x, 1, 3, 62).reshape(-1)[3 * 32:].reshape(32, 5)
    assert want[0].tolist() == [2, 0, 0, 0, 0] and want[1].tolist() == [0, 3, 0, 0, 0]
    assert want[2].tolist() == [0, 0, 0, 4, 0] and want[3].tolist() == [0, 0, 0, 0, 5]
    neg = -np.abs(_map(np.random.RandomState(7), 2 * 3 * 62, 32)) - 0.5
    assert not _tpp(neg, 2, 3, 62).any()


def test_tpp_max_element_path_and_other_levels():
    x = _map(np.random.RandomState(8), 2 * 3 * 9, 30)
    _tpp(x, 2, 3, 9, ld=33, col=1)
    _tpp(x, 2, 3, 9, levels=(3, 1, 16, 2), ld=33, col=2)
    x = _map(np.random.RandomState(9), 2 * 3 * 9, 260)   # more than one run of 64 four-channel units, the last one ragged
    _tpp(x, 2, 3, 9, levels=(2, 7))


def test_tpp_max_refusals():
    lib, p = N.lib(), 4096
    lv = (C.c_int32 * 9)(1, 2, 5, 1, 1, 1, 1, 1, 1)
    ok = dict(x=p, ld=32, batch=1, h=2, w=4, c=32, levels=C.addressof(lv), n=3, f=p, ld_out=256, hi=p, lo=p, ld_pl=256)
    z, big = (C.c_int32 * 2)(1, 0), (C.c_int32 * 2)(1, 17)
    bad = [dict(x=None), dict(levels=None), dict(f=None, hi=None, lo=None), dict(hi=None), dict(batch=0), dict(w=0), dict(c=0),
           dict(ld=31), dict(n=0), dict(n=9), dict(levels=C.addressof(z), n=2), dict(levels=C.addressof(big), n=2), dict(ld_out=255),
           dict(ld_pl=255)]
    for kw in bad:
        a = dict(ok)
        a.update(kw)
        assert lib.wd_tpp_max(a["x"], a["ld"], a["batch"], a["h"], a["w"], a["c"], a["levels"], a["n"], a["f"], a["ld_out"], a["hi"],
                              a["lo"], a["ld_pl"], _st()) == N.WD_EINVAL, kw


# ---- wd_resize_bilinear ----------------------------------------------------------------------------------------------------
def _resize(x, h, w, bgr=False, ld_in=None, ld_out=None, col=0):
    B, Cc, hs, ws = x.shape
    xbuf, xv = G.pitched(torch.from_numpy(x.reshape(-1, ws)), ws if ld_in is None else ld_in, col, device=DEV)
    obuf, ov = G.guarded(B * Cc * h, w, w if ld_out is None else ld_out, col, torch.float32, device=DEV)
    rc = N.lib().wd_resize_bilinear(xv.data_ptr(), xbuf.shape[-1], B, Cc, hs, ws, ov.data_ptr(), obuf.shape[-1], h, w, int(bgr), _st())
    assert rc == N.WD_OK
    torch.cuda.synchronize()
    G.assert_untouched(xbuf, xv, "x")
    G.assert_untouched(obuf, ov, "out")
    G.assert_finite(ov, "out")
    got = ov.cpu().reshape(B, Cc, h, w)
    assert torch.equal(got, torch.from_numpy(R.resize_np(x, h, w, bgr)))
    return got


@pytest.mark.parametrize("hs,ws,h,w", [(64, 256, 50, 250), (7, 9, 5, 4), (5, 4, 7, 9)])
def test_resize_bilinear_bit_for_bit(hs, ws, h, w):
    x = np.random.RandomState(10).random_sample((2, 3, hs, ws)).astype(np.float32)
    a = _resize(x, h, w)
    b = _resize(x, h, w, ld_in=ws + 5, ld_out=w + 3, col=1)  # the element path: the same bits
    assert torch.equal(a, b)
    flipped = _resize(x, h, w, bgr=True)
    assert torch.equal(flipped, a.flip(1))


def test_resize_bilinear_same_size_is_the_identity():
    x = np.random.RandomState(11).random_sample((2, 3, 6, 8)).astype(np.float32)
    assert torch.equal(_resize(x, 6, 8), torch.from_numpy(x))
    assert torch.equal(_resize(x, 6, 8, bgr=True), torch.from_numpy(x).flip(1))


def test_resize_bilinear_refusals():
    lib, p = N.lib(), 4096
    for kw in (dict(x=None), dict(out=None), dict(batch=0), dict(c=0), dict(hs=0), dict(w=0), dict(ld_in=7), dict(ld_out=3),
               dict(h=1 << 23)):
        a = dict(x=p, ld_in=8, batch=1, c=3, hs=4, ws=8, out=p, ld_out=4, h=2, w=4)
        a.update(kw)
        assert lib.wd_resize_bilinear(a["x"], a["ld_in"], a["batch"], a["c"], a["hs"], a["ws"], a["out"], a["ld_out"], a["h"], a["w"], 0,
                                      _st()) == N.WD_EINVAL, kw


# ---- wd_phosc_finish -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ld_phos,ld_phoc,ld_out", [(165, 604, 769), (192, 640, 772), (171, 611, 775)])
def test_phosc_finish(ld_phos, ld_phoc, ld_out):
    rs = np.random.RandomState(12)
    phos = _map(rs, 5, 165)
    phoc = (rs.standard_normal((5, 604)) * 6.0).astype(np.float32)
    phoc[0, :4] = [0.0, -0.0, 40.0, -40.0]
    phoc[1, :2] = [100.0, -100.0]   # exp overflows to inf: the quotient is 0, not NaN
    abuf, av = G.pitched(torch.from_numpy(phos), ld_phos, 0, device=DEV)
    bbuf, bv = G.pitched(torch.from_numpy(phoc), ld_phoc, ld_phoc - 604, device=DEV)
    obuf, ov = G.guarded(5, 769, ld_out, ld_out - 769, torch.float32, device=DEV)
    assert N.lib().wd_phosc_finish(av.data_ptr(), ld_phos, 165, bv.data_ptr(), ld_phoc, 604, 5, ov.data_ptr(), ld_out, _st()) == N.WD_OK
    torch.cuda.synchronize()
    for name, (buf, view) in dict(phos=(abuf, av), phoc=(bbuf, bv), out=(obuf, ov)).items():
        G.assert_untouched(buf, view, name)
    G.assert_finite(ov, "out")
    want = R.finish_np(phos, phoc)
    got = ov.cpu().numpy()
    assert np.array_equal(got[:, :165], want[:, :165].astype(np.float32)) and not np.signbit(got[:, :165]).any()
    err = float(np.abs(got[:, 165:].astype(np.float64) - want[:, 165:]).max())
    print(f"wd_phosc_finish: sigmoid max abs error {err:.3e}")
    assert err <= 1e-6


def test_phosc_finish_refusals():
    lib, p = N.lib(), 4096
    for kw in (dict(phos=None), dict(phoc=None), dict(out=None), dict(batch=0), dict(n1=0), dict(n2=0), dict(ld1=164), dict(ld2=603),
               dict(ldo=768)):
        a = dict(phos=p, ld1=165, n1=165, phoc=p, ld2=604, n2=604, batch=1, out=p, ldo=769)
        a.update(kw)
        assert lib.wd_phosc_finish(a["phos"], a["ld1"], a["n1"], a["phoc"], a["ld2"], a["n2"], a["batch"], a["out"], a["ldo"],
                                   _st()) == N.WD_EINVAL, kw


# ---- wd_phosc_score --------------------------------------------------------------------------------------------------------
def _score_case(B=5, V=37, D=769, seed=13):
    rs = np.random.RandomState(seed)
    table = rs.random_sample((V, D)).astype(np.float32)
    table *= rs.random_sample((V, D)) < 0.3            # non-negative and sparse, like PHOSC vectors
    rows = rs.permutation(V)[:B] if B <= V else rs.randint(0, V, B)
    pred = (table[rows] * rs.uniform(0.5, 2.0, (B, 1)) + 0.05 * rs.standard_normal((B, D))).astype(np.float32)
    return pred, table, rows


def _score64(pred, table):
    p, t = torch.from_numpy(pred).double(), torch.from_numpy(table).double()
    s = (p @ t.T) / torch.clamp(p.norm(dim=1)[:, None] * t.norm(dim=1)[None, :], min=1e-8)
    return s.numpy()


def _score(pred, table, target=None, want=("scores", "best_idx", "best_score", "target_score"), ld_pred=None, ld_table=None, col=0,
           use_ws=False):
    B, D = pred.shape
    V = table.shape[0]
    pbuf, pv = G.pitched(torch.from_numpy(pred), D if ld_pred is None else ld_pred, col, device=DEV)
    tbuf, tv = G.pitched(torch.from_numpy(table), D if ld_table is None else ld_table, col, device=DEV)
    norm = torch.from_numpy(table).double().norm(dim=1).float()
    nbuf, nv = G.guarded_flat(V, torch.float32, device=DEV)
    nv.copy_(norm)
    sbuf, sv = G.guarded(B, V, V + 3, 2, torch.float32, device=DEV)
    ibuf, iv = G.guarded_flat(B, torch.int32, device=DEV)
    bbuf, bv = G.guarded_flat(B, torch.float32, device=DEV)
    cbuf, cv = G.guarded_flat(B, torch.float32, device=DEV)
    wbuf, wv = G.guarded_flat(B * V, torch.float32, device=DEV)
    tgt = None
    if target is not None:
        gbuf, tgt = G.guarded_flat(B, torch.int32, device=DEV)
        tgt.copy_(torch.as_tensor(target, dtype=torch.int32))
    ptr = lambda name, t: t.data_ptr() if name in want else None  # noqa: E731
    rc = N.lib().wd_phosc_score(pv.data_ptr(), pbuf.shape[-1], B, D, tv.data_ptr(), tbuf.shape[-1], nv.data_ptr(), V,
                                ptr("scores", sv), V + 3, ptr("best_idx", iv), ptr("best_score", bv),
                                tgt.data_ptr() if tgt is not None else None, ptr("target_score", cv) if tgt is not None else None,
                                wv.data_ptr() if use_ws else None, _st())
    assert rc == N.WD_OK
    torch.cuda.synchronize()
    outs = dict(scores=(sbuf, sv), best_idx=(ibuf, iv), best_score=(bbuf, bv), target_score=(cbuf, cv))
    for name, (buf, view) in dict(pred=(pbuf, pv), table=(tbuf, tv), norm=(nbuf, nv), **outs).items():
        if name in want or name not in outs:
            G.assert_untouched(buf, view, name)
        else:  # an output that was passed nowhere keeps the pattern in every element
            assert bool((buf.view(torch.int32) == G.NAN32).all()), name
    if not use_ws:
        assert bool((wbuf.view(torch.int32) == G.NAN32).all()), "ws was passed nowhere"
    return {name: view.cpu().numpy() for name, (buf, view) in outs.items() if name in want}


@pytest.mark.parametrize("ld,col", [(772, 0), (769, 0), (775, 3)])   # the 16-byte path with its tail lane, the element path twice
def test_phosc_score_against_float64(ld, col):
    pred, table, rows = _score_case()
    ref = _score64(pred, table)
    top2 = np.sort(ref, axis=1)[:, -2:]
    assert float((top2[:, 1] - top2[:, 0]).min()) > 1e-2   # (a condition of the construction)
    assert np.array_equal(ref.argmax(1), rows)
    target = [int(rows[0]), -1, 37, 3, 36]
    got = _score(pred, table, target, ld_pred=ld, ld_table=ld, col=col)
    err = float(np.abs(got["scores"].astype(np.float64) - ref).max())
    print(f"wd_phosc_score ld {ld}: max abs error {err:.3e}")
    assert err <= 1e-4
    assert np.array_equal(got["best_idx"], ref.argmax(1).astype(np.int32))
    assert np.array_equal(got["best_score"], got["scores"][np.arange(5), got["best_idx"]])
    ts = got["target_score"]
    assert np.isnan(ts[1]) and np.isnan(ts[2]) and ts[0] == got["scores"][0, rows[0]] and ts[3] == got["scores"][3, 3] \
        and ts[4] == got["scores"][4, 36]
    spec = R.score_np(pred, table, None, target)
    assert float(np.abs(spec[0].astype(np.float64) - ref).max()) <= 1e-4 and np.array_equal(spec[1], got["best_idx"])


def test_phosc_score_first_maximum_and_small_tables():
    pred, table, rows = _score_case(B=3, V=300, seed=14)   # more than one block of 64 words, more words than threads of the scan
    table[200] = table[rows[0]]
    table[7] = table[rows[1]]
    got = _score(pred, table, ld_pred=772, ld_table=772)
    assert got["best_idx"][0] == min(200, rows[0]) and got["best_idx"][1] == min(7, rows[1]) and got["best_idx"][2] == rows[2]
    assert np.array_equal(got["best_idx"], R.first_max(got["scores"]))
    one = _score(pred, table[:1].copy(), [0, 0, 0], ld_pred=772, ld_table=772)
    assert one["best_idx"].tolist() == [0, 0, 0] and np.array_equal(one["best_score"], one["scores"][:, 0])
    assert np.array_equal(one["target_score"], one["scores"][:, 0])
    zero = _score(np.zeros((2, 769), np.float32), table[:5].copy(), ld_pred=772, ld_table=772)  # |x| = 0: the 1e-8 floor, not NaN
    assert not zero["scores"].any() and zero["best_idx"].tolist() == [0, 0]


def test_phosc_score_every_output_is_optional():
    pred, table, rows = _score_case()
    full = _score(pred, table, rows, ld_pred=772, ld_table=772)
    for want in (("scores",), ("best_idx",), ("best_score",), ("target_score",), ("best_idx", "target_score")):
        got = _score(pred, table, rows, want=want, ld_pred=772, ld_table=772, use_ws="scores" not in want)
        for name in want:
            assert np.array_equal(got[name], full[name]), (want, name)
    assert np.array_equal(full["target_score"], full["best_score"])


def test_phosc_score_refusals():
    lib, p = N.lib(), 4096
    ok = dict(pred=p, ldp=772, batch=2, d=769, table=p, ldt=772, norm=p, v=5, scores=p, lds=5, bi=p, bs=p, ti=p, ts=p, ws=None)
    bad = [dict(pred=None), dict(table=None), dict(norm=None), dict(batch=0), dict(d=0), dict(v=0), dict(ldp=768), dict(ldt=768),
           dict(lds=4), dict(ti=None), dict(scores=None), dict(scores=None, bi=None, bs=None, ts=None, ws=p)]
    for kw in bad:
        a = dict(ok)
        a.update(kw)
        assert lib.wd_phosc_score(a["pred"], a["ldp"], a["batch"], a["d"], a["table"], a["ldt"], a["norm"], a["v"], a["scores"], a["lds"],
                                  a["bi"], a["bs"], a["ti"], a["ts"], a["ws"], _st()) == N.WD_EINVAL, kw
