"""The batched form of the 64-row tile epilogue (wd_epilogue_rows, csrc/wd_gemm_epi.h): a thread's row loads in one round trip, then
its rows' arithmetic and stores.  It is the row loop's arithmetic in the row loop's order, so every case launches twice through the
C ABI - dbg WD_EPI_BATCH_ON (the batched form wherever wd_epilogue_batch_ok finds it legal) and dbg WD_EPI_BATCH_OFF (the row loop, what
WDIFF_EPI_BATCH=0 runs) - and asks for

  * the same BITS in out_f32, both planes and stat_part;
  * the resolved dbg bit WD_EPI_BATCH_BIT on the first launch only (else the loop is compared with itself);
  * the batched result against the fp64 reference with the bounds of tests/test_gpu_gemmw_slab.py (result and planes rel_err < 2e-5,
    statistics max_rel < 1e-5), so that two equal wrong answers do not pass.

Shapes, the smallest at which the row sequence can go wrong: n = 320, c = 64 (k = 576); tile 64320 on an 8 x 8 map at B = 2 (two
tiles, one sample each) and an 8 x 32 map at B = 1 (four tiles inside one sample), slab and per-tap kernel; tile 64080 on a 4 x 16 map
at B = 2; wd_ff_fused at m = 128, hw_out = 64, inner = 256 on its plain, proj_out and folded tails, and the transformer front at
B = 1.  Launches the predicate refuses (ragged m, two samples per panel, GEGLU, a resid_rows table) must resolve to the loop and
return its bits; one pitched, guard-banded case checks that nothing outside a tile's own columns is written."""
import ctypes as C
import types

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests import _guard as G  # noqa: E402
from tests._common import FULL, make_args, max_rel, rel_err  # noqa: E402
from tests.test_gpu_pitch import DENSE, _case, _conv, _ff_pack, _geglu_case, _launch, _linear, _pitch, _run, _st, _sync, _unpl  # noqa: E402
from worddiffusion_amd import UNetModel  # noqa: E402
from worddiffusion_amd import _native as N  # noqa: E402
from worddiffusion_amd.engine import geglu_interleave  # noqa: E402
from worddiffusion_amd.synthetic import fill_module_, synthetic_inputs  # noqa: E402

DEV = "cuda:0"
EPI_ON, EPI_OFF = N.EPI_BATCH_ON, N.EPI_BATCH_OFF   # wd_gemm_args.dbg / wd_ff_args.dbg: override WDIFF_EPI_BATCH; resolved EPI_ON = batched form taken
SLAB_ON, SLAB_OFF = N.GEMMW_SLAB_ON, N.GEMMW_SLAB_OFF


def _both(cs_kw, P, batched=True, dbg=0):
    """The case under both switches: (forced-on launch, forced-off launch), each asserted to have resolved to its form."""
    runs = []
    for bit in (EPI_ON, EPI_OFF):
        got = _launch(_case(**dict(cs_kw, dbg=dbg | bit)), P)
        assert got.kernel == cs_kw["kernel"], f"the case is about {cs_kw['kernel']}, wd_gemm runs it on {got.kernel}"
        assert bool(got.resolved[6] & EPI_ON) == (batched and bit == EPI_ON), f"dbg {bit:#x} resolved to {got.resolved}"
        assert not got.resolved[6] & EPI_OFF and got.vec_path   # (the bit names the form of the 16-byte path: the launch must be on it)
        runs.append(got)
    return runs


def _same_bits(tag, on, off):
    assert set(on.win) == set(off.win)
    for key in on.win:
        G.assert_finite(on.win[key], f"{tag}: {key}")
        assert torch.equal(on.win[key], off.win[key]), f"{tag}: {key} of the batched form differs from the row loop's"


def _against_fp64(tag, cs_kw, on):
    ref, fig = cs_kw["ref"], {}
    if "out" in on.win:
        fig["out"] = rel_err(on.win["out"].cpu(), ref)
    if "pl" in on.win:
        fig["planes"] = rel_err(_unpl(on.win["pl"]), ref)
    if "stat" in on.win:
        B, hw, cpg = cs_kw["m"] // cs_kw["hw_out"], cs_kw["hw_out"], cs_kw["stat_cpg"]
        o = ref.reshape(B, hw, ref.shape[1] // cpg, cpg)
        st = on.win["stat"].cpu().reshape(B, -1, ref.shape[1] // cpg, 2).sum(1)
        fig["stat"] = max(max_rel(st[..., 0], o.sum(dim=(1, 3))), max_rel(st[..., 1], (o * o).sum(dim=(1, 3))))
    print(f"{tag}: " + ", ".join(f"{k} {v:.3g}" for k, v in fig.items()))
    assert fig.get("out", 0) < 2e-5 and fig.get("planes", 0) < 2e-5 and fig.get("stat", 0) < 1e-5


_OPERANDS = {"bias": dict(film=False, resid=False), "bias + FiLM": dict(film=True, resid=False), "bias + resid": dict(film=False, resid=True)}
_OUTPUTS = {"f32": dict(f32=True, planes=False), "planes": dict(f32=False, planes=True), "f32 + planes": dict(f32=True, planes=True)}
# (kernel, tile, map height, width, samples, dbg of the launch: the slab form / the per-tap form of the 64 x 320 kernel)
_TILES = {
    "64320 slab, 8 x 8, B 2": ("K_GEMMW", 64320, 8, 8, 2, SLAB_ON),
    "64320 slab, 8 x 32, B 1": ("K_GEMMW", 64320, 8, 32, 1, SLAB_ON),
    "64320 per-tap, 8 x 8, B 2": ("K_GEMMW", 64320, 8, 8, 2, SLAB_OFF),
    "64080, 4 x 16, B 2": ("K_GEMMQ", 64080, 4, 16, 2, 0),
}


@pytest.mark.parametrize("operands", sorted(_OPERANDS))
@pytest.mark.parametrize("shape", sorted(_TILES))
def test_batched_form_returns_the_bits_of_the_row_loop(shape, operands):
    kernel, tile, hh, ww, B, dbg = _TILES[shape]
    d = _conv(320, c1=64, c2=0, hh=hh, ww=ww, B=B, **_OPERANDS[operands])
    for stat_cpg in (0, 10):
        for outs, okw in _OUTPUTS.items():
            kw = dict(d, kernel=kernel, tile=tile, w_layout=3, slab_rows=ww, stat_cpg=stat_cpg, **okw)
            tag = f"{shape}, {operands}, stat {stat_cpg}, {outs}"
            on, off = _both(kw, DENSE, dbg=dbg)
            _same_bits(tag, on, off)
            _against_fp64(tag, kw, on)


def test_batched_form_with_silu():
    """SiLU is the one activation the batched form serves (the FiLM tables of the sampler run it): a linear layer, m = 128."""
    d = _linear(128, 64, 320)
    kw = dict(d, hw_out=64, act=N.ACT_SILU, ref=F.silu(d["ref"]), kernel="K_GEMMW", tile=64320, w_layout=3)
    on, off = _both(kw, DENSE)
    _same_bits("SiLU", on, off)
    _against_fp64("SiLU", kw, on)


def _rows_case():
    g = torch.Generator().manual_seed(91)
    m, k, n = 128, 64, 320
    a, w = torch.randn(m, k, generator=g), torch.randn(n, k, generator=g) / 8
    bias, table = torch.randn(n, generator=g), torch.randn(11, n, generator=g)
    y = torch.randint(0, 11, (m,), generator=g, dtype=torch.int64)
    ref = a.double() @ w.double().t() + bias.double() + table[y].double()
    return dict(srcs=[(a, k, 1, None, 0)], w=w, m=m, hw_out=64, bias=bias, resid=table, resid_rows=y, ref=ref, kernel="K_GEMMW", tile=64320,
                w_layout=3)


_REFUSED = {
    "m = 96: the last tile is ragged": lambda: dict(_linear(96, 64, 320), hw_out=64, kernel="K_GEMMW", tile=64320, w_layout=3),
    "hw_out = 32, B = 4: two samples per panel, with statistics": lambda: dict(_conv(320, c1=64, c2=0, hh=4, ww=8, B=4), kernel="K_GEMMW",
                                                                              tile=64320, w_layout=3, slab_rows=8, stat_cpg=10),
    "GEGLU": lambda: vars(_geglu_case(64064)),
    "a resid_rows table": _rows_case,
}


@pytest.mark.parametrize("name", sorted(_REFUSED))
def test_launches_the_predicate_refuses_run_the_row_loop(name):
    kw = _REFUSED[name]()
    kw = {k: v for k, v in kw.items() if k != "dbg"}
    on, off = _both(kw, DENSE, batched=False)
    assert on.resolved == off.resolved
    _same_bits(name, on, off)


def test_batched_form_on_a_pitched_guarded_output():
    """out_ld = n + 8, out_pl_ld = n + 8, resid_ld = n + 4, every operand a window of a NaN-filled buffer with guard rows: a store
    outside a tile's own columns changes the pattern, a read outside an operand's window brings a NaN in."""
    P = _pitch(out=(8, 4), pl=(8, 4), resid=(4, 4))
    d = _conv(320, c1=64, c2=0, hh=8, ww=8, B=2)
    kw = dict(d, kernel="K_GEMMW", tile=64320, w_layout=3, slab_rows=8, stat_cpg=10)
    on, off = _both(kw, P, dbg=SLAB_ON)
    for got in (on, off):
        for name, buf, view in got.outs:
            G.assert_untouched(buf, view, name)
    _same_bits("pitched", on, off)
    _against_fp64("pitched", kw, on)
    dense = _both(kw, DENSE, dbg=SLAB_ON)[0]
    for key in on.win:
        assert torch.equal(on.win[key], dense.win[key]), f"{key}: the pitched launch differs from the dense one"


# ---- wd_ff_fused
def _ff_data(m=128, inner=256):
    c = 320
    g = torch.Generator().manual_seed(m + inner)
    d = dict(m=m, inner=inner, x=torch.randn(m, c, generator=g))
    w1, b1 = torch.randn(2 * inner, c, generator=g) / c ** 0.5, torch.randn(2 * inner, generator=g)
    w2, w3 = torch.randn(c, inner, generator=g) / inner ** 0.5, torch.randn(c, c, generator=g) / c ** 0.5
    d.update(b2=torch.randn(c, generator=g), b3=torch.randn(c, generator=g), res=torch.randn(m, c, generator=g), res3=torch.randn(m, c, generator=g))
    d.update(w1=geglu_interleave(w1, 16), b1=geglu_interleave(b1, 16), w2=w2, w3=w3)
    xd = d["x"].double()
    hid = (xd @ w1[:inner].double().t() + b1[:inner].double()) * F.gelu(xd @ w1[inner:].double().t() + b1[inner:].double())
    d["ref"] = d["res"].double() + hid @ w2.double().t() + d["b2"].double()
    d["ref3"] = d["res3"].double() + d["ref"] @ w3.double().t() + d["b3"].double()
    return d


def _ff_launch(d, tail, stat, dbg, P=DENSE):
    """wd_ff_fused on the plain tail, the proj_out tail or the folded tail (W32 = W3 W2 by wd_linear_fold, as the engine derives it),
    hw_out = 64: the windows, everything the launch may write, and the dbg wd_ff_check resolved."""
    c, m, inner, g = 320, d["m"], d["inner"], P.g
    a = N.WdFfArgs()
    xb, xv = G.pitched_planes(d["x"], c + P.src[0], P.src[1], g, DEV)
    a.x_hi, a.x_lo, a.x_ld = xv[0].data_ptr(), xv[1].data_ptr(), xb.shape[-1]
    a.m, a.c, a.inner, a.npass, a.hw_out, a.dbg = m, c, inner, 3, 64, dbg
    packs = [_ff_pack(d[nm]) for nm in ("w1", "w2", "w3")]
    vecs = [d[nm].to(DEV) for nm in ("b1", "b2", "b3")]
    a.w1_hi, a.w1_lo, a.b1 = packs[0][0].data_ptr(), packs[0][1].data_ptr(), vecs[0].data_ptr()
    a.w2_hi, a.w2_lo, a.b2 = packs[1][0].data_ptr(), packs[1][1].data_ptr(), vecs[1].data_ptr()
    rb, rv = G.pitched(d["res"], c + P.resid[0], P.resid[1], g, DEV)
    a.resid, a.resid_ld = rv.data_ptr(), rb.shape[-1]
    obuf, out = G.guarded(m, c, c + P.out[0], P.out[1], torch.float32, g, DEV)
    pbuf, pl = G.guarded(m, c, c + P.pl[0], P.pl[1], torch.bfloat16, g, DEV, planes=2)
    a.out_f32, a.out_ld = out.data_ptr(), obuf.shape[-1]
    a.out_hi, a.out_lo, a.out_pl_ld = pl[0].data_ptr(), pl[1].data_ptr(), pbuf.shape[-1]
    outs, win, keep = [("out_f32", obuf, out), ("out planes", pbuf, pl)], dict(out=out, pl=pl), [xb, rb, packs, vecs]
    if tail != "plain":
        r3b, r3v = G.pitched(d["res3"], c + P.rowvec[0], P.rowvec[1], g, DEV)
        a.w3_hi, a.w3_lo, a.b3 = packs[2][0].data_ptr(), packs[2][1].data_ptr(), vecs[2].data_ptr()
        a.resid3, a.resid3_ld = r3v.data_ptr(), r3b.shape[-1]
        keep.append(r3b)
    if tail == "folded":
        w3d, w2d = d["w3"].to(DEV), d["w2"].to(DEV)
        w32, b32 = torch.empty(c, inner, device=DEV), torch.empty(c, device=DEV)
        _run("wd_linear_fold", w3d.data_ptr(), w2d.data_ptr(), vecs[1].data_ptr(), vecs[2].data_ptr(), c, c, inner, w32.data_ptr(),
             b32.data_ptr(), _st())
        _sync()
        p32 = _ff_pack(w32.cpu())
        a.w32_hi, a.w32_lo, a.b32 = p32[0].data_ptr(), p32[1].data_ptr(), b32.data_ptr()
        keep += [p32, b32]
    if stat:
        sbuf, part = G.guarded(m // 64, 64, 64, 0, torch.float64, g, DEV)
        a.stat_part, a.stat_cpg = part.data_ptr(), c // 32
        outs.append(("stat_part", sbuf, part))
        win["stat"] = part
    r = N.WdFfArgs()
    assert N.lib().wd_ff_check(C.byref(a), C.byref(r)) == N.WD_OK
    _run("wd_ff_fused", C.byref(a), _st())
    _sync()
    return types.SimpleNamespace(win=win, outs=outs, keep=keep, dbg=r.dbg)


@pytest.mark.parametrize("stat", [False, True])
@pytest.mark.parametrize("tail", ["plain", "proj_out", "folded"])
def test_ff_fused_batched_form_returns_the_bits_of_the_row_loop(tail, stat):
    d = _ff_data()
    want = d["ref"] if tail == "plain" else d["ref3"]
    on, off = (_ff_launch(d, tail, stat, bit) for bit in (EPI_ON, EPI_OFF))
    assert on.dbg & EPI_ON and not off.dbg & (EPI_ON | EPI_OFF), f"resolved {on.dbg:#x} / {off.dbg:#x}"
    _same_bits(f"ff {tail}", on, off)
    _against_fp64(f"ff {tail}, stat {stat}", dict(ref=want, m=d["m"], hw_out=64, stat_cpg=10), on)


def test_ff_fused_batched_form_on_a_pitched_guarded_output():
    d = _ff_data()
    P = _pitch(src=(8, 8), out=(8, 4), pl=(8, 4), resid=(4, 4), rowvec=(4, 4))
    on, dense = _ff_launch(d, "proj_out", True, EPI_ON, P), _ff_launch(d, "proj_out", True, EPI_ON)
    assert on.dbg & EPI_ON
    for name, buf, view in on.outs:
        G.assert_untouched(buf, view, name)
    _same_bits("ff pitched", on, dense)


def test_ff_fused_front_batched_form_returns_the_bits_of_the_row_loop():
    """The transformer front of one 8 x 32 sample (four panels): out, statistics and tok2 under both switches."""
    from tests.test_gpu_st_fused import _Block
    blk = _Block(1)
    res = []
    for bit in (EPI_ON, EPI_OFF):
        out = torch.full((blk.m, blk.c), float("nan"), device=DEV)
        stat = torch.full((blk.B, blk.hw // 64, 32, 2), float("nan"), dtype=torch.float64, device=DEV)
        tok2 = torch.full((blk.m, blk.c), float("nan"), device=DEV)
        f = blk.fused_args(out, stat, tok2)
        f.dbg = bit
        r = N.WdFfArgs()
        assert blk.lib.wd_ff_check(C.byref(f), C.byref(r)) == N.WD_OK and bool(r.dbg & EPI_ON) == (bit == EPI_ON)
        _run("wd_ff_fused", C.byref(f), _st())
        _sync()
        res.append((out, stat, tok2))
    for x, y in zip(*res):
        assert torch.isfinite(x).all() and torch.equal(x, y)


# ---- the engine
def test_engine_switch_and_the_step_plan(monkeypatch):
    """FULL base forward at B = 64, WDIFF_EPI_BATCH=1 against 0: the same bits, and with the switch on the plan's ten 64 x 320 launches
    (seven wd_gemm on tile 64320, three wd_ff_fused) all resolve to the batched form, with the switch off none does."""
    inp = synthetic_inputs(64, seed=5)
    outs = []
    for on in ("0", "1"):
        monkeypatch.setenv("WDIFF_EPI_BATCH", on)
        m = UNetModel(args=make_args(device=DEV, phosc=0), **FULL)
        fill_module_(m, 2)
        m = m.to(DEV).eval()
        assert m.engine.epi_batch == (on == "1")
        with torch.no_grad():
            outs.append(m(inp["x"].to(DEV), None, original_images=None, timesteps=inp["t"].to(DEV), context=inp["context"].to(DEV),
                          y=inp["y"].to(DEV)))
        lib, wide, ff = m.engine.lib, [], []
        for P in m.engine._plans.values():
            for fn, args, _what in P.step:
                a = getattr(args[0], "_obj", args[0]) if args else None
                if fn.__name__ == "wd_gemm":
                    r = N.WdGemmArgs()
                    assert lib.wd_gemm_check(C.byref(a), C.byref(r)) == N.WD_OK
                    if r.tile == 64320:
                        wide.append(bool(r.dbg & EPI_ON))
                elif fn.__name__ == "wd_ff_fused":
                    r = N.WdFfArgs()
                    assert lib.wd_ff_check(C.byref(a), C.byref(r)) == N.WD_OK
                    ff.append(bool(r.dbg & EPI_ON))
        print(f"WDIFF_EPI_BATCH={on}: 64 x 320 wd_gemm launches {wide}, wd_ff_fused {ff}")
        assert len(wide) == 7 and len(ff) == 3 and all(x == (on == "1") for x in wide + ff)
        del m
    assert torch.isfinite(outs[1]).all()
    assert torch.equal(outs[0], outs[1]), "the batched epilogue changed the forward's bits"
