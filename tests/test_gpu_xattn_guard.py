"""The folded cross-attention (csrc/wd_xattn.hip: wd_xattn_fold and its consumers wd_xattn_fused in both forms, wd_xattn_pair,
wd_xattn_planes with and without the second layer) behind guard bands (tests/_guard.py), at every border of heads * L, and on
staircase logits.

wd_xattn_fold: K / V two windows of one pitched buffer (K at column 4, V at column c + 12, NaN between, around, and in the rows
before the first sample and after the last), mq / mo contiguous runs between poisoned pads, mq_pl / mot_pl zero-initialised (as the
header requires) between poisoned pads.  mq / mo against fp64 (2e-5); the planes are, element for element, the bf16 split of mq / mo
at the fragment-major position the kernels read it from, and every other element is still zero.

The consumers: x a window with ld = c + 8, out / n_hi, n_lo / r_hi, r_lo windows with the pitches c + 12 / c + 8 / c + 4.  out
against fp64 (2e-5), the LayerNorm planes (3e-5), the raw planes bit for bit split_planes(out), the guarded launch bit for bit the
dense launch, nothing written outside, and the same bits in the planes that remain with n_lo = NULL and with r_lo = NULL.

heads * L takes 1 (a softmax of one key), 16, 17, 32, 33 and 40: the borders of the three 16-row score tiles and of the two 32-pair
output k-steps of xattn16_kernel; hw takes 1, 15, 16, 17 and 70 (its 16-token tiles, the 64-token tiles of xattn_fused_kernel).

out == x is not a case: the engine never passes it (engine.py: _st_attn_folded and _st_attn_pair write fresh buffers from the
rows they read; _transformer_fused does not call these entry points at all).

Largest max_rel against fp64 seen on an MI355X (out / LayerNorm planes; tolerances 2e-5 / 3e-5):
  xattn_fold_kernel        the seven shapes: mq 6.3e-07, mo 5.9e-07
  xattn_fused_kernel       every shape (form 'valu'), both staircase cases                  2.3e-07 / 6.3e-06
  xattn16_kernel<NP = 1>   every shape (forms 'mfma', 'planes'), both staircase cases       2.5e-06 / 6.3e-06
  xattn16_kernel<NP = 2>   every shape (forms 'pair', 'pair+planes')                        1.5e-06 / 5.4e-06"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _attn_ref as R  # noqa: E402
from tests import _guard as G  # noqa: E402
from worddiffusion_amd import _native as N  # noqa: E402

DEV = "cuda:0"
TOL_F32, TOL_PL = 2e-5, 3e-5
XHJ = 64  # csrc/wd_xattn.hip: (head, key) pairs of the plane images


def _st():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def mq_index(hj, n, c):
    """xa_mq_index of csrc/wd_xattn.hip: Mq plane [64 hj][c], fragment-major for the B operand of v_mfma_f32_16x16x32_bf16."""
    return (((hj >> 4) * (c >> 5) + (n >> 5)) << 9) + ((((n >> 3) & 3) * 16 + (hj & 15)) << 3) + (n & 7)


def mo_index(n, hj):
    """xa_mo16_index: Mo^T plane [c][64 hj]."""
    return (((n >> 4) * 2 + (hj >> 5)) << 9) + ((((hj >> 3) & 3) * 16 + (n & 15)) << 3) + (hj & 7)


@functools.lru_cache(maxsize=None)
def _operands(B, hw, c, heads, L, seed=0, step=0, period=1):
    """Operands of one layer and its fp64 results (mq, mo, out, ln): computed once, shared, never modified."""
    o = R.xattn_operands(B, hw, c, heads, L, seed=seed, step=step, period=period)
    return o, R.xattn_fp64(o, B, hw, c, heads, L)


def fold(o, B, c, heads, L):
    """wd_xattn_fold behind guard bands -> dict(mq, mo: fp32 windows [B][heads * L][c]; mq_pl, mot_pl: windows [B][2][64 * c]) on
    the device, the pads checked."""
    lib = N.lib()
    d, HJ = c // heads, heads * L
    ld = 2 * c + 16
    kv = G.poisoned((B * L + 4, ld), torch.float32)
    kv[2:2 + B * L, 4:4 + c] = o["k"]
    kv[2:2 + B * L, c + 12:2 * c + 12] = o["v"]
    kv = kv.to(DEV)
    wq, wo = o["wq"].to(DEV), o["wo"].to(DEV)
    bufs = {}
    for name, n, dt in (("mq", B * HJ * c, torch.float32), ("mo", B * HJ * c, torch.float32),
                        ("mq_pl", B * 2 * XHJ * c, torch.bfloat16), ("mot_pl", B * 2 * XHJ * c, torch.bfloat16)):
        bufs[name] = G.guarded_flat(n, dt, device=DEV)
        if dt == torch.bfloat16:
            bufs[name][1].zero_()
    N.check(lib.wd_xattn_fold(kv[2, 4:].data_ptr(), ld, kv[2, c + 12:].data_ptr(), ld, B, heads, L, d, float(d ** -0.5), wq.data_ptr(),
                              wo.data_ptr(), c, *(bufs[n][1].data_ptr() for n in ("mq", "mo", "mq_pl", "mot_pl")), _st()),
            "wd_xattn_fold")
    torch.cuda.synchronize()
    for name, (buf, view) in bufs.items():
        G.assert_untouched(buf, view, f"wd_xattn_fold {name} (c={c}, heads={heads}, L={L})")
        G.assert_finite(view, f"wd_xattn_fold {name}")
    return dict(mq=bufs["mq"][1].view(B, HJ, c), mo=bufs["mo"][1].view(B, HJ, c), mq_pl=bufs["mq_pl"][1].view(B, 2, XHJ * c),
                mot_pl=bufs["mot_pl"][1].view(B, 2, XHJ * c), keep=(bufs, kv, wq, wo))


# (c, heads, L, hw): heads * L = 1, 16, 17, 32, 33, 40, 40, two more token counts, and d = 160 at the model's 10 keys (--num_heads 2)
SHAPES = [(64, 1, 1, 1), (64, 4, 4, 15), (64, 1, 17, 16), (64, 2, 16, 17), (320, 1, 33, 70), (320, 4, 10, 17), (320, 8, 5, 16),
          (64, 4, 4, 70), (320, 4, 10, 1), (320, 2, 10, 17)]


@pytest.mark.parametrize("c,heads,L,hw", SHAPES[:7])
def test_fold_behind_guard_bands(c, heads, L, hw):
    B, HJ = 2, heads * L
    lib = N.lib()
    assert lib.wd_xattn_supported(c, heads, L) == 1
    o, (mq, mo, _, _) = _operands(B, hw, c, heads, L)
    f = fold(o, B, c, heads, L)
    e_mq, e_mo = R.max_rel(f["mq"].cpu(), mq), R.max_rel(f["mo"].cpu(), mo)
    print(f"ERR xattn_fold_kernel (c={c}, heads={heads}, L={L}): mq {e_mq:.2e} mo {e_mo:.2e}")
    assert e_mq < TOL_F32 and e_mo < TOL_F32
    # the planes: the split of the fp32 matrices at the fragment-major positions, zero everywhere else
    hj, n = torch.meshgrid(torch.arange(HJ), torch.arange(c), indexing="ij")
    for name, idx, src in (("mq_pl", mq_index(hj, n, c), f["mq"]), ("mot_pl", mo_index(n, hj), f["mo"])):
        assert int(idx.max()) < XHJ * c and idx.unique().numel() == HJ * c
        want = torch.zeros(B, 2, XHJ * c, dtype=torch.bfloat16)
        want[:, :, idx.reshape(-1)] = G.split_planes(src.cpu()).permute(1, 0, 2, 3).reshape(B, 2, HJ * c)
        got = f[name].cpu()
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"{name}: not the split of the fp32 matrix in place"
    # ... and by difference: folded again from zeroed planes with other K / V, the positions that are zero in both hi planes are
    # exactly the padding (nothing but the heads * L live rows was addressed)
    o2 = dict(o, k=o["k"] * 0.7 + 0.11, v=o["v"] * 1.3 - 0.07)
    f2 = fold(o2, B, c, heads, L)
    for name in ("mq_pl", "mot_pl"):
        a, b = f[name].cpu().view(torch.int16), f2[name].cpu().view(torch.int16)
        live = (a[:, 0] != 0) | (b[:, 0] != 0)
        assert int(live.sum()) == B * HJ * c, f"{name}: {int(live.sum())} elements addressed, {B * HJ * c} expected"
        assert not bool(((a[:, 1] != 0) & ~live).any()) and not bool(((b[:, 1] != 0) & ~live).any())
    assert lib.wd_xattn_fold(None, 4, None, 4, B, heads, L, c // heads, 1.0, None, None, c, None, None, None, None, _st()) == N.WD_EINVAL


def _dev(o):
    return {n: t.contiguous().to(DEV) for n, t in o.items()}


def consume(form, x, layers, folds, B, hw, c, heads, L, dense=False, n_lo=True, r_lo=True):
    """One consumer launch.  form: 'valu' / 'mfma' (wd_xattn_fused without / with the plane images), 'planes' (wd_xattn_planes, one
    layer, raw planes), 'pair' (wd_xattn_pair), 'pair+planes' (wd_xattn_planes, two layers, raw planes).  layers: device operand
    dicts; folds: fold() results.  Returns host (out [B * hw][c], n planes, r planes or None); asserts nothing else changed."""
    lib = N.lib()
    rows = B * hw
    g = 0 if dense else 2

    def win(extra, col0, dtype, planes=0):
        return G.guarded(rows, c, c + (0 if dense else extra), 0 if dense else col0, dtype, g, DEV, planes)

    xbuf, xv = win(8, 4, torch.float32)
    xv.copy_(x)
    obuf, ov = win(12, 4, torch.float32)
    nbuf, nv = win(8, 4, torch.bfloat16, 2)
    rbuf, rv = win(4, 0, torch.bfloat16, 2)
    a = layers[0]
    ln2 = (a["ga2"].data_ptr(), a["be2"].data_ptr(), 1e-5, nv[0].data_ptr(), nv[1].data_ptr() if n_lo else None, nbuf.shape[-1])
    raw = form in ("planes", "pair+planes")
    if form in ("valu", "mfma"):
        pl = (folds[0]["mq_pl"].data_ptr(), folds[0]["mot_pl"].data_ptr()) if form == "mfma" else (None, None)
        N.check(lib.wd_xattn_fused(xv.data_ptr(), xbuf.shape[-1], B, hw, c, a["ga"].data_ptr(), a["be"].data_ptr(), 1e-5,
                                   folds[0]["mq"].data_ptr(), folds[0]["mo"].data_ptr(), heads, L, a["bo"].data_ptr(), ov.data_ptr(),
                                   obuf.shape[-1], *ln2, *pl, _st()), "wd_xattn_fused")
    else:
        def lay(ly, fo):
            return (ly["ga"].data_ptr(), ly["be"].data_ptr(), fo["mq_pl"].data_ptr(), fo["mot_pl"].data_ptr(), ly["bo"].data_ptr())
        second = lay(layers[1], folds[1]) if form.startswith("pair") else (None,) * 5
        args = (xv.data_ptr(), xbuf.shape[-1], B, hw, c, 1e-5, heads, L, *lay(a, folds[0]), *second, ov.data_ptr(), obuf.shape[-1], *ln2)
        if form == "pair":
            N.check(lib.wd_xattn_pair(*args, _st()), "wd_xattn_pair")
        else:
            N.check(lib.wd_xattn_planes(*args, rv[0].data_ptr(), rv[1].data_ptr() if r_lo else None, rbuf.shape[-1], _st()),
                    "wd_xattn_planes")
    torch.cuda.synchronize()
    what = f"{form} (c={c}, heads={heads}, L={L}, hw={hw}{', dense' if dense else ''})"
    G.assert_untouched(xbuf, xv, "x " + what)
    G.assert_untouched(obuf, ov, "out " + what)
    G.assert_untouched(nbuf[0], nv[0], "n_hi " + what)
    G.assert_untouched(nbuf[1], nv[1] if n_lo else (0, 0, 0, 0), "n_lo " + what)
    G.assert_untouched(rbuf[0], rv[0] if raw else (0, 0, 0, 0), "r_hi " + what)
    G.assert_untouched(rbuf[1], rv[1] if raw and r_lo else (0, 0, 0, 0), "r_lo " + what)
    G.assert_finite(ov, "out " + what)
    G.assert_finite(nv if n_lo else nv[0], "n planes " + what)
    if raw:
        G.assert_finite(rv if r_lo else rv[0], "r planes " + what)
    return ov.cpu(), nv.cpu(), (rv.cpu() if raw else None)


def check_consumers(B, hw, c, heads, L, step=0, period=1, forms=("valu", "mfma", "planes", "pair", "pair+planes")):
    oa, (_, _, out_a, ln_a) = _operands(B, hw, c, heads, L, 0, step, period)
    ob = dict(_operands(B, hw, c, heads, L, 1, step, period)[0])
    ob["x"], ob["ga2"], ob["be2"] = out_a.float(), oa["ga2"], oa["be2"]   # the second layer reads the first one's result
    _, _, out_b, ln_b = R.xattn_fp64(dict(ob, x=out_a), B, hw, c, heads, L)
    layers = [_dev(oa), _dev(ob)]
    folds = [fold(oa, B, c, heads, L), fold(ob, B, c, heads, L)]
    x = oa["x"]
    errs = {}
    for form in forms:
        ref, ref_n = (out_b, ln_b) if form.startswith("pair") else (out_a, ln_a)
        out, npl, rpl = consume(form, x, layers, folds, B, hw, c, heads, L)
        e, en = R.max_rel(out, ref), R.max_rel(npl[0].float() + npl[1].float(), ref_n)
        kern = "xattn_fused_kernel" if form == "valu" else f"xattn16_kernel<NP={2 if form.startswith('pair') else 1}>"
        print(f"ERR {kern} {form} (c={c}, heads={heads}, L={L}, hw={hw}, step={step}): out {e:.2e} planes {en:.2e}")
        assert e < TOL_F32 and en < TOL_PL
        errs[form] = (e, en)
        if rpl is not None:
            assert torch.equal(rpl.view(torch.int16), G.split_planes(out).view(torch.int16)), "raw planes != split_planes(out)"
        od, nd, rd = consume(form, x, layers, folds, B, hw, c, heads, L, dense=True)
        assert torch.equal(od, out) and torch.equal(nd, npl) and (rpl is None or torch.equal(rd, rpl))
        o1, n1, r1 = consume(form, x, layers, folds, B, hw, c, heads, L, n_lo=False, r_lo=False)
        assert torch.equal(o1, out) and torch.equal(n1[0], npl[0]) and (rpl is None or torch.equal(r1[0], rpl[0]))
    return errs


@pytest.mark.parametrize("c,heads,L,hw", SHAPES)
def test_folded_consumers_behind_guard_bands(c, heads, L, hw):
    """xattn_fused_kernel ('valu'), xattn16_kernel<NP = 1> ('mfma', 'planes'), xattn16_kernel<NP = 2> ('pair', 'pair+planes'); c = 64
    and c = 320 both have single-layer and pair cases with the raw planes (r_hi / r_lo), which no other test writes."""
    check_consumers(2, hw, c, heads, L)


@pytest.mark.parametrize("B,hw,c,heads,L,step,period", R.XATTN_STAIRCASE)
def test_folded_consumers_on_staircase_logits(B, hw, c, heads, L, step, period):
    """L = 10, the stairs put into K before wd_xattn_fold (tests/_attn_ref.py xattn_operands): logits spanning 7 and 63 nats through
    the fold, both forms of the fused kernel and the plane-writing one."""
    check_consumers(B, hw, c, heads, L, step, period, forms=("valu", "mfma", "planes"))


def test_folded_entry_points_refuse_what_they_cannot_run():
    lib = N.lib()
    assert lib.wd_xattn_supported(64, 4, 11) == 0 and lib.wd_xattn_supported(128, 4, 10) == 0 and lib.wd_xattn_supported(64, 3, 10) == 0
    B, hw, c, heads, L = 1, 4, 64, 4, 10
    z = torch.zeros(8 * 64 * c, device=DEV)
    zb = torch.zeros(2 * 2 * 64 * c, dtype=torch.bfloat16, device=DEV)
    p, pb = z.data_ptr(), zb.data_ptr()
    fused = lambda ld, out_ld, n_ld, hl: lib.wd_xattn_fused(p, ld, B, hw, c, p, p, 1e-5, p, p, heads, hl, p, p, out_ld, p, p, 1e-5,  # noqa: E731
                                                            pb, pb, n_ld, None, None, _st())
    assert fused(c + 2, c, c, L) == N.WD_EINVAL and fused(c, c + 2, c, L) == N.WD_EINVAL and fused(c, c, c + 2, L) == N.WD_EINVAL
    assert fused(c, c, c, 11) == N.WD_EINVAL
    lay = (p, p, pb, pb, p)
    planes = lambda r_ld, r_hi, r_lo: lib.wd_xattn_planes(p, c, B, hw, c, 1e-5, heads, L, *lay, None, None, None, None, None, p, c, p, p,  # noqa: E731
                                                         1e-5, pb, pb, c, r_hi, r_lo, r_ld, _st())
    assert planes(c + 2, pb, pb) == N.WD_EINVAL and planes(c, None, pb) == N.WD_EINVAL
    assert lib.wd_xattn_pair(p, c, B, hw, c, 1e-5, heads, L, *lay, p, p, None, pb, p, p, c, p, p, 1e-5, pb, pb, c, _st()) == N.WD_EINVAL
    torch.cuda.synchronize()
    assert not bool(z.any()) and not bool(zb.any())
