"""The GEMM family (wd_gemm, wd_ff_fused) and the plane producers that feed it on PITCHED operands: every operand a window of a
wider, taller buffer (tests/_guard.py) whose every other element is a NaN pattern.  Each case launches twice - dense (every pitch
equal to the width, outputs exactly m x n) and pitched - resolved to the same kernel (wd_gemm_check / wd_gemm_check_kernel), and
checks the pitched window against the fp64 reference (tolerances of tests/test_gpu_kernels.py: npass-3 GEMM results and their
planes 2e-5 rel_err, GroupNorm / LayerNorm planes 3e-5 max_rel, statistics 1e-5; wd_ff_fused - two chained GEMMs - 3e-5 as its
own test there), against the dense launch (the same bits where both take the same epilogue path, max_rel 5e-6 where the pitched
launch is forced onto the scalar epilogue), for finiteness (a read outside an operand's window brings a NaN in) and every
output buffer, workspace and ticket array for stores outside its window."""
import ctypes as C
import functools
import types

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests import _guard as G  # noqa: E402
from tests._common import max_rel, rel_err  # noqa: E402
from worddiffusion_amd import _native as N  # noqa: E402
from worddiffusion_amd.engine import conv_gather_table, geglu_interleave  # noqa: E402

DEV = "cuda:0"
FORMS = ("K_V1", "K_V2", "K_M16", "K_V4", "K_GEMMW", "K_GEMMQ")


def _st():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _run(name, *args):
    N.check(getattr(N.lib(), name)(*args), name)


def _sync():
    torch.cuda.synchronize()


# ---- pitch variants: (extra columns, window column) per operand; g = guard rows before and after
def _pitch(g=2, src=(24, 8), out=(12, 4), pl=(8, 4), resid=(4, 4), rowvec=(8, 4), a32=(12, 4), vec=(0, 0), exact=True):
    return types.SimpleNamespace(g=g, src=src, out=out, pl=pl, resid=resid, rowvec=rowvec, a32=a32, vec=vec, exact=exact)


DENSE = _pitch(0, (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0))
PITCH = {
    "a": _pitch(),                                  # padded, multiples of 4 and 8: the vector epilogue
    # n = 70 with every pitch a multiple of 4 (out 84, planes 80, resid 76, row vector 80; windows at column 4): the vector
    # epilogue, whose last float4 of a row (columns 68..71) is ragged.  The dense launch (out_ld = 70) takes the scalar epilogue.
    "b": _pitch(out=(14, 4), pl=(10, 4), resid=(6, 4), rowvec=(10, 4), exact=False),
    "c": _pitch(out=(1, 0), pl=(3, 1), exact=False),  # odd pitches: the scalar epilogue
    "d": _pitch(out=(12, 1), exact=False),          # fp32 window off the 16-byte grid: the scalar epilogue
}


def _case(**kw):
    d = dict(hw_out=1, bias=None, rowvec=None, resid=None, resid_rows=None, act=0, tile=0, ksplit=1, dbg=0, w_layout=0, slab_rows=0,
             tickets=False, f32=True, planes=True, lo=True, stat_cpg=0, gn=None, ln=None, a32=None, w_embed=None, inplace=None,
             ref_planes=None, kernel=None)
    d.update(kw)
    return types.SimpleNamespace(**d)


def _launch(cs, P):
    """One wd_gemm launch of case cs with the pitches P.  Returns the windows, (name, buffer, window) of everything the launch may
    write, and what wd_gemm_check resolved."""
    lib = N.lib()
    a = N.WdGemmArgs()
    keep, outs = [], []
    g = P.g
    for i, (x, c, ntaps, gather, hw_src) in enumerate(cs.srcs):
        s = N.WdSrc()
        if i == 0 and cs.a32 is not None:
            buf, view = G.pitched(x, c + P.a32[0], P.a32[1], g, DEV)
            B = cs.m // cs.hw_out
            nchunk = lib.wd_gn_nchunk(hw_src)
            ngr = c // cs.a32["cpg"]
            pbuf, part = G.guarded(B * nchunk, ngr * 2, ngr * 2, 0, torch.float64, g, DEV)
            _run("wd_gn_stats", view.data_ptr(), buf.shape[-1], B, hw_src, c, cs.a32["cpg"], part.data_ptr(), _st())
            outs.append(("a32 statistics", pbuf, part))
            gam, bet = G.pitched(cs.a32["gamma"][None], c, 0, g, DEV)[1], G.pitched(cs.a32["beta"][None], c, 0, g, DEV)[1]
            a.a32, a.a32_ld, a.a32_part = view.data_ptr(), buf.shape[-1], part.data_ptr()
            a.a32_nchunk, a.a32_pcpg, a.a32_cpg = nchunk, cs.a32["cpg"], cs.a32["cpg"]
            a.a32_gamma, a.a32_beta, a.a32_eps, a.a32_silu = gam.data_ptr(), bet.data_ptr(), cs.a32["eps"], cs.a32["silu"]
            keep += [buf, gam, bet]
            s.ld = c
        else:
            buf, view = G.pitched_planes(x, c + P.src[0], P.src[1], g, DEV)
            keep.append(buf)
            s.hi, s.lo, s.ld = view[0].data_ptr(), view[1].data_ptr(), buf.shape[-1]
        if gather is not None:
            tab = torch.from_numpy(gather).to(DEV)
            keep.append(tab)
            s.gather = tab.data_ptr()
        s.c, s.ntaps, s.hw_src = c, ntaps, hw_src
        a.src[i] = s
    a.nsrc, a.npass = len(cs.srcs), 3
    n, ktot = cs.w.shape
    if cs.w_embed and g:  # a run of rows of a taller matrix: NaN rows before and after
        wb, wv = G.pitched_planes(cs.w, ktot, 0, cs.w_embed, DEV)
        wp = wv
        keep.append(wb)
    else:
        wp = G.split_planes(cs.w).to(DEV)
    if cs.w_layout == 3:
        wf = torch.empty_like(wp)
        _run("wd_gemm_pack_w", wp[0].data_ptr(), wp[1].data_ptr(), n, ktot, wf[0].data_ptr(), wf[1].data_ptr(), _st())
        wp = wf
    keep.append(wp)
    a.w_hi, a.w_lo, a.w_layout, a.slab_rows = wp[0].data_ptr(), wp[1].data_ptr(), cs.w_layout, cs.slab_rows
    a.m, a.n, a.ktot, a.hw_out = cs.m, n, ktot, cs.hw_out
    a.act, a.tile, a.ksplit, a.dbg = cs.act, cs.tile, cs.ksplit, cs.dbg
    n_out = n // 2 if cs.act == N.ACT_GEGLU else n

    def vec(v, pad=(0, 0)):  # a per-column vector: one row, guard rows around it
        t = G.pitched(v[None], v.numel() + pad[0], pad[1], g, DEV)[1]
        keep.append(t)
        return t.data_ptr()

    if cs.bias is not None:
        a.bias = vec(cs.bias)
    if cs.rowvec is not None:
        buf, view = G.pitched(cs.rowvec, n_out + P.rowvec[0], P.rowvec[1], g, DEV)
        keep.append(buf)
        a.rowvec, a.rowvec_ld = view.data_ptr(), buf.shape[-1]
    win = {}
    if cs.f32:
        obuf, out = G.guarded(cs.m, n_out, n_out + P.out[0], P.out[1], torch.float32, g, DEV)
        if cs.inplace is not None:  # accumulate in place: resid == out_f32
            out.copy_(cs.inplace)
            a.resid, a.resid_ld = out.data_ptr(), obuf.shape[-1]
        a.out_f32, a.out_ld = out.data_ptr(), obuf.shape[-1]
        outs.append(("out_f32", obuf, out))
        win["out"] = out
    if cs.resid is not None:
        buf, view = G.pitched(cs.resid, n_out + P.resid[0], P.resid[1], g, DEV)
        keep.append(buf)
        a.resid, a.resid_ld = view.data_ptr(), buf.shape[-1]
    if cs.resid_rows is not None:
        rr = cs.resid_rows.to(DEV)
        keep.append(rr)
        a.resid_rows = rr.data_ptr()
    if cs.planes:
        pbuf, pl = G.guarded(cs.m, n_out, n_out + P.pl[0], P.pl[1], torch.bfloat16, g, DEV, planes=2)
        a.out_hi, a.out_pl_ld = pl[0].data_ptr(), pbuf.shape[-1]
        if cs.lo:
            a.out_lo = pl[1].data_ptr()
            outs.append(("out planes", pbuf, pl))
        else:
            outs.append(("out_hi", pbuf[0], pl[0]))
            outs.append(("the lo plane (out_lo NULL)", pbuf[1], (0, 0, 0, 0)))
        win["pl"] = pl
    if cs.stat_cpg:
        bm = cs.tile // 1000
        nchunk = max(1, cs.hw_out // (bm if cs.w_layout == 3 else 128))
        ngr = n // cs.stat_cpg
        sbuf, part = G.guarded((cs.m // cs.hw_out) * nchunk, ngr * 2, ngr * 2, 0, torch.float64, g, DEV)
        a.stat_part, a.stat_cpg = part.data_ptr(), cs.stat_cpg
        outs.append(("stat_part", sbuf, part))
        win["stat"] = part
    if cs.gn is not None:
        a.gn_gamma, a.gn_beta = vec(cs.gn["gamma"], P.vec), vec(cs.gn["beta"], P.vec)
        a.gn_eps, a.gn_silu, a.gn_cpg = cs.gn["eps"], cs.gn["silu"], cs.gn["cpg"]
    if cs.ln is not None:
        a.ln_gamma, a.ln_beta, a.ln_eps = vec(cs.ln["gamma"]), vec(cs.ln["beta"]), cs.ln["eps"]
    if cs.ksplit != 1:
        wbuf, ws = G.guarded(cs.ksplit * cs.m, n, n, 0, torch.float32, g, DEV)
        a.ws, a.ws_floats = ws.data_ptr(), ws.numel()
        outs.append(("ws", wbuf, ws))
    tk = None
    if cs.tickets:
        tbuf, tk = G.guarded(1, 64, 64, 0, torch.int32, g, DEV)
        tk.zero_()
        a.tickets, a.ntickets = tk.data_ptr(), tk.numel()
        outs.append(("tickets", tbuf, tk))
    res = N.WdGemmArgs()
    assert lib.wd_gemm_check(C.byref(a), C.byref(res)) == N.WD_OK, "wd_gemm_check refuses the case"
    kern = lib.wd_gemm_check_kernel(C.byref(a)).decode()
    resolved = (kern, res.tile, res.ksplit, bool(res.tickets), res.slab_rows, res.w_layout, res.dbg)
    # the epilogue's 16-byte path (wd_epilogue_vec_ok): pitches % 4, fp32 operands 16-byte and planes 8-byte aligned
    vec_path = (not (a.out_ld | a.rowvec_ld | a.resid_ld | a.out_pl_ld) & 3 and
                not ((a.bias or 0) | (a.rowvec or 0) | (a.resid or 0) | (a.out_f32 or 0)) & 15 and not ((a.out_hi or 0) | (a.out_lo or 0)) & 7)
    _run("wd_gemm", C.byref(a), _st())
    _sync()
    if tk is not None:
        assert int(tk.abs().sum()) == 0, "tickets not left zeroed"
    return types.SimpleNamespace(win=win, outs=outs, resolved=resolved, kernel=kern, keep=keep, vec_path=vec_path)


def _unpl(p):
    return p[0].float().cpu().double() + p[1].float().cpu().double()


def _check(cs, P, tag=""):
    """The four steps of every case: dense launch, pitched launch on the same kernel, window check, guard check."""
    dense, got = _launch(cs, DENSE), _launch(cs, P)
    assert got.resolved == dense.resolved, f"dense and pitched launches resolve differently: {dense.resolved} / {got.resolved}"
    assert got.kernel == cs.kernel, f"the case is about {cs.kernel}, wd_gemm runs it on {got.kernel}"
    for name, buf, view in got.outs:
        G.assert_untouched(buf, view, f"{tag}{name}")
    for key, w in got.win.items():
        if key == "pl" and not cs.lo:
            w = w[0]
        G.assert_finite(w, f"{tag}{key} window")
    fig = {}
    if cs.f32:
        fig["out"] = rel_err(got.win["out"].cpu(), cs.ref)
    if cs.planes and cs.lo:
        pref = cs.ref if cs.ref_planes is None else cs.ref_planes
        fig["planes"] = (rel_err if cs.ref_planes is None else max_rel)(_unpl(got.win["pl"]), pref)
    if cs.stat_cpg:
        B, ngr = cs.m // cs.hw_out, cs.w.shape[0] // cs.stat_cpg
        st = got.win["stat"].cpu().reshape(B, -1, ngr, 2).sum(1)
        o = cs.ref.reshape(B, cs.hw_out, ngr, cs.stat_cpg)
        fig["stat"] = max(max_rel(st[..., 0], o.sum(dim=(1, 3))), max_rel(st[..., 1], (o * o).sum(dim=(1, 3))))
    for key in got.win:
        d, p = dense.win[key], got.win[key]
        if key == "pl" and not cs.lo:
            d, p = d[0], p[0]
        if P.exact:
            assert torch.equal(d, p), f"{tag}{key}: the pitched launch differs from the dense one on the same epilogue path"
        else:
            d, p = (_unpl(d), _unpl(p)) if key == "pl" else (d.cpu(), p.cpu())
            fig[key + " vs dense"] = max_rel(p, d)
    print(f"{tag}{got.resolved}: " + ", ".join(f"{k} {v:.3g}" for k, v in fig.items()))
    assert fig.get("out", 0) < 2e-5 and fig.get("planes", 0) < (2e-5 if cs.ref_planes is None else 3e-5) and fig.get("stat", 0) < 1e-5
    assert all(v < 5e-6 for k, v in fig.items() if k.endswith("vs dense"))
    if cs.planes and not cs.lo:  # hi alone: bf16 of the value
        pref = cs.ref if cs.ref_planes is None else cs.ref_planes
        assert max_rel(got.win["pl"][0].float().cpu(), pref) < 2.0 ** -8
    return got


# ---- shapes: one linear and one 3x3 + identity-skip (B = 3 samples of 8 x 8 or 4 x 16: hw = 64, m = 192)
@functools.lru_cache(maxsize=None)
def _linear(m, k, n, seed=0):
    g = torch.Generator().manual_seed(1000 * m + k + n + seed)
    a, w = torch.randn(m, k, generator=g), torch.randn(n, k, generator=g) / k ** 0.5
    bias, res = torch.randn(n, generator=g), torch.randn(m, n, generator=g)
    ref = a.double() @ w.double().t() + bias.double() + res.double()
    return dict(srcs=[(a, k, 1, None, 0)], w=w, m=m, bias=bias, resid=res, ref=ref)


@functools.lru_cache(maxsize=None)
def _conv(n, c1=64, c2=128, hh=8, ww=8, B=3, film=True, resid=True, seed=0):
    g = torch.Generator().manual_seed(n + c1 + c2 + ww + seed)
    hw, m = hh * ww, B * hh * ww
    a1 = torch.randn(m, c1, generator=g)
    tab, _, _ = conv_gather_table(hh, ww, "same")
    w = torch.randn(n, 9 * c1 + c2, generator=g) / (9 * c1 + c2) ** 0.5
    bias, rv, res = torch.randn(n, generator=g), torch.randn(B, n, generator=g), torch.randn(m, n, generator=g)
    x1 = a1.reshape(B, hh, ww, c1).permute(0, 3, 1, 2)
    ref = (F.conv2d(x1.double(), w[:, :9 * c1].reshape(n, 3, 3, c1).permute(0, 3, 1, 2).double(), padding=1)
           .permute(0, 2, 3, 1).reshape(m, n) + bias.double())
    srcs = [(a1, c1, 9, tab, hw)]
    if c2:
        a2 = torch.randn(m, c2, generator=g)
        ref = ref + a2.double() @ w[:, 9 * c1:].double().t()
        srcs.append((a2, c2, 1, None, 0))
    d = dict(srcs=srcs, w=w, m=m, hw_out=hw, bias=bias, ref=ref)
    if film:
        d["rowvec"], d["ref"] = rv, d["ref"] + rv.double().repeat_interleave(hw, 0)
    if resid:
        d["resid"], d["ref"] = res, d["ref"] + res.double()
    return d


# name: (kernel form, shape(n) -> case fields, n per variant)
_N100 = dict(a=100, b=70, c=100, d=100)
_FORMS = {
    "V1 linear": ("K_V1", lambda n: dict(_linear(130, 96, n), tile=128064), _N100),
    "V1 3x3 + skip": ("K_V1", lambda n: dict(_conv(n, 96, 32), tile=128064), _N100),
    "V2 128x64 linear": ("K_V2", lambda n: dict(_linear(130, 64, n), tile=128064), _N100),
    "V2 64x64 linear": ("K_V2", lambda n: dict(_linear(130, 64, n), tile=64064), _N100),
    "V2 128x64 3x3 + skip": ("K_V2", lambda n: dict(_conv(n), tile=128064), _N100),
    "V2 64x64 3x3 + skip": ("K_V2", lambda n: dict(_conv(n), tile=64064), _N100),
    "M16 linear": ("K_M16", lambda n: dict(_linear(130, 128, n), tile=128160), dict(a=160, c=160, d=160)),
    "M16 3x3 + skip, ragged n": ("K_M16", lambda n: dict(_conv(n), tile=128160), dict(a=200, c=200, d=200)),
    "V4 linear": ("K_V4", lambda n: dict(_linear(130, 128, n), tile=128160, dbg=N.DBG_FORCE_V4), dict(a=160, c=160, d=160)),
    "V4 3x3 + skip": ("K_V4", lambda n: dict(_conv(n), tile=128160, dbg=N.DBG_FORCE_V4), dict(a=160, c=200, d=160)),
    "W 64x320 linear": ("K_GEMMW", lambda n: dict(_linear(130, 64, n), tile=64320, w_layout=3), dict(a=320, c=320, d=320)),
    "W 64x320 3x3 + skip": ("K_GEMMW", lambda n: dict(_conv(n), tile=64320, w_layout=3), dict(a=320, c=320, d=320)),
    "W 64x320 3x3 + skip, computed rows": ("K_GEMMW", lambda n: dict(_conv(n), tile=64320, w_layout=3, slab_rows=8), dict(a=320, c=320, d=320)),
    "W 128x160 3x3 + skip": ("K_GEMMW", lambda n: dict(_conv(n), tile=128160, w_layout=3), dict(a=160, c=160, d=160)),
    "W 128x160 3x3 + skip, computed rows": ("K_GEMMW", lambda n: dict(_conv(n), tile=128160, w_layout=3, slab_rows=8), dict(a=160, c=160, d=160)),
    "Q linear": ("K_GEMMQ", lambda n: dict(_linear(192, 128, n), hw_out=64, tile=64080, w_layout=3), dict(a=160, c=160, d=160)),
    "Q 3x3 + skip, 4x16": ("K_GEMMQ", lambda n: dict(_conv(n, hh=4, ww=16), tile=64080, w_layout=3, slab_rows=16), dict(a=160, c=160, d=160)),
}
_FORM_CASES = [(name, v) for name, (_, _, ns) in _FORMS.items() for v in sorted(ns)]


def test_the_table_covers_every_kernel_form():
    """Each case below asserts the kernel wd_gemm_check_kernel resolved; together they name every form wd_gemm ships by default."""
    assert {k for k, _, _ in _FORMS.values()} == set(FORMS)


@pytest.mark.parametrize("name,variant", _FORM_CASES)
def test_gemm_forms_on_pitched_operands(name, variant):
    """Every kernel form x pitch variant: (a) padded pitches - the vector epilogue; (b) n = 70 inside pitches that are multiples
    of 4 - the ragged float4 of the vector epilogue, against a dense launch that can only take the scalar one (5e-6, not the same
    bits); (c) odd pitches and (d) an fp32 window off the 16-byte grid - the scalar epilogue."""
    kernel, make, ns = _FORMS[name]
    if variant == "b":  # the premise of (b): n % 4 != 0, every epilogue pitch % 4 == 0
        P, n = PITCH["b"], ns["b"]
        assert n % 4 and not any((n + e) % 4 or c0 % 4 for e, c0 in (P.out, P.pl, P.resid, P.rowvec))
    got = _check(_case(kernel=kernel, **make(ns[variant])), PITCH[variant], f"{name} ({variant}): ")
    assert got.vec_path == (variant in "ab"), "the pitched launch is not on the epilogue path this variant is about"


# ---- epilogue features, pitch variant (a)
def _silu_rows_case(tile):
    g = torch.Generator().manual_seed(77)
    m, k, n = 130, 64, 100
    a, w = torch.randn(m, k, generator=g), torch.randn(n, k, generator=g) / 8
    bias, table = torch.randn(n, generator=g), torch.randn(11, n, generator=g)
    y = torch.randint(0, 11, (m,), generator=g, dtype=torch.int64)
    ref = F.silu(a.double() @ w.double().t() + bias.double() + table[y].double())
    return _case(srcs=[(a, k, 1, None, 0)], w=w, m=m, bias=bias, resid=table, resid_rows=y, act=N.ACT_SILU, tile=tile, ref=ref, kernel="K_V2")


def _geglu_case(tile):
    g = torch.Generator().manual_seed(78)
    m, dim, inner = 130, 64, 128
    a, w = torch.randn(m, dim, generator=g), torch.randn(2 * inner, dim, generator=g) / dim ** 0.5
    b, res = torch.randn(2 * inner, generator=g), torch.randn(m, inner, generator=g)
    h = a.double() @ w.double().t() + b.double()
    ref = h[:, :inner] * F.gelu(h[:, inner:]) + res.double()
    gr = (tile % 1000) // 2
    return _case(srcs=[(a, dim, 1, None, 0)], w=geglu_interleave(w, gr), m=m, bias=geglu_interleave(b, gr), resid=res, act=N.ACT_GEGLU,
                 tile=tile, ref=ref, kernel="K_V2")


def _ln_case():
    d = _linear(130, 64, 320, seed=3)
    g = torch.Generator().manual_seed(79)
    gam, bet = torch.randn(320, generator=g) * 0.3 + 1, torch.randn(320, generator=g) * 0.2
    refn = F.layer_norm(d["ref"], (320,), gam.double(), bet.double(), 1e-5)
    return _case(**d, tile=64320, w_layout=3, ln=dict(gamma=gam, beta=bet, eps=1e-5), ref_planes=refn, kernel="K_GEMMW")


def _a32_case(c2, silu):
    g = torch.Generator().manual_seed(80 + c2)
    B, hh, ww, cin, n = 3, 8, 8, 64, 320
    hw, m, cpg = hh * ww, B * hh * ww, 2
    x = torch.randn(m, cin, generator=g) * 1.5 + 0.3
    gam, bet = torch.randn(cin, generator=g) * 0.3 + 1, torch.randn(cin, generator=g) * 0.2
    w = torch.randn(n, 9 * cin + c2, generator=g) / (9 * cin + c2) ** 0.5
    bias = torch.randn(n, generator=g)
    xn = F.group_norm(x.double().reshape(B, hw, cin).permute(0, 2, 1), cin // cpg, gam.double(), bet.double(), 1e-5)
    xn = F.silu(xn) if silu else xn
    ref = F.conv2d(xn.reshape(B, cin, hh, ww), w[:, :9 * cin].reshape(n, 3, 3, cin).permute(0, 3, 1, 2).double(), padding=1)
    ref = ref.permute(0, 2, 3, 1).reshape(m, n) + bias.double()
    tab, _, _ = conv_gather_table(hh, ww, "same")
    srcs = [(x, cin, 9, tab, hw)]
    if c2:
        a2 = torch.randn(m, c2, generator=g)
        ref = ref + a2.double() @ w[:, 9 * cin:].double().t()
        srcs.append((a2, c2, 1, None, 0))
    return _case(srcs=srcs, w=w, m=m, hw_out=hw, bias=bias, ref=ref, tile=64320, w_layout=3, slab_rows=ww,
                 a32=dict(gamma=gam, beta=bet, cpg=cpg, eps=1e-5, silu=silu), kernel="K_GEMMW")


_FEATURES = {
    "FiLM row vector, V2": lambda: _case(kernel="K_V2", **dict(_conv(100, resid=False), tile=128064)),
    "FiLM row vector, M16": lambda: _case(kernel="K_M16", **dict(_conv(160, resid=False), tile=128160)),
    "resid_rows + SiLU, 128x64": lambda: _silu_rows_case(128064),
    "resid_rows + SiLU, 64x64": lambda: _silu_rows_case(64064),
    "GEGLU, 128x64": lambda: _geglu_case(128064),
    "GEGLU, 64x64": lambda: _geglu_case(64064),
    "statistics, M16": lambda: _case(kernel="K_M16", **dict(_conv(160), tile=128160, stat_cpg=5)),
    "statistics, V2 128x64": lambda: _case(kernel="K_V2", **dict(_conv(128), tile=128064, stat_cpg=4)),
    "statistics, W 64x320": lambda: _case(kernel="K_GEMMW", **dict(_conv(320), tile=64320, w_layout=3, stat_cpg=10)),
    "statistics, W 128x160": lambda: _case(kernel="K_GEMMW", **dict(_conv(160), tile=128160, w_layout=3, stat_cpg=5)),
    "statistics, Q": lambda: _case(kernel="K_GEMMQ", **dict(_conv(160, hh=4, ww=16), tile=64080, w_layout=3, slab_rows=16, stat_cpg=5)),
    "ln on 64x320": _ln_case,
    "a32 staging": lambda: _a32_case(0, 1),
    "a32 staging + identity source": lambda: _a32_case(128, 0),
}


@pytest.mark.parametrize("name", sorted(_FEATURES))
def test_gemm_epilogue_features_on_pitched_operands(name):
    _check(_FEATURES[name](), PITCH["a"], name + ": ")


def test_gemm_run_of_weight_rows_into_a_column_slice():
    """The data-gradient form: w_hi / w_lo point at a run of rows of a taller matrix (NaN rows before and after the run), n is
    the run's length, the result goes to a column slice of a wider output."""
    d = _conv(100, seed=9)
    for tile, kern in ((128064, "K_V2"), (64064, "K_V2"), (128160, "K_M16")):
        _check(_case(kernel=kern, w_embed=16, planes=False, **dict(d, tile=tile)), _pitch(out=(156, 40)), f"rows 16..116, tile {tile}: ")
    dv = _conv(100, 96, 32, seed=9)
    _check(_case(kernel="K_V1", w_embed=16, planes=False, **dict(dv, tile=128064)), _pitch(out=(156, 40)), "rows 16..116, V1: ")


# ---- K cut: the separate combine launch and the in-launch combine (tickets + dbg WD_DBG_FORCE_TICKETS)
def _gn_ref(ref, hw, cpg, gam, bet, eps, silu):
    m, n = ref.shape
    y = F.group_norm(ref.reshape(m // hw, hw, n).permute(0, 2, 1), n // cpg, gam.double(), bet.double(), eps)
    y = F.silu(y) if silu else y
    return y.permute(0, 2, 1).reshape(m, n)


@pytest.mark.parametrize("tickets", [False, True])
@pytest.mark.parametrize("ksplit", [2, 3])
@pytest.mark.parametrize("name", ["direct, n 160", "image, n 100", "scalar slabs, n 70", "flat in place", "W 64x320", "W 128x160"])
def test_gemm_k_cut_on_pitched_operands(name, ksplit, tickets):
    """The combine of a K cut by branch: n = 160 sums the slabs inside the vector epilogue; n = 100 stages its ragged last 64 x 40
    combine tile (columns 80..119) through the LDS image; n = 70 (odd pitches) stores and sums the slabs element by element; fp32-only
    output with resid == out_f32 accumulates in place (reference acc0 + A W^T + bias) - in the flat combine launch, and with tickets
    inside the GEMM's own epilogue.  wd_gemm keeps the tickets only for whole column tiles on the LDS-staged kernels: the
    tickets = True runs of the other cases assert that they resolve to the combine launch."""
    kw = dict(ksplit=ksplit, tickets=tickets, dbg=N.DBG_FORCE_TICKETS if tickets else 0)
    if name == "direct, n 160":
        cs = _case(kernel="K_M16", **dict(_conv(160), tile=128160, **kw))
    elif name == "image, n 100":
        cs = _case(kernel="K_V2", **dict(_conv(100), tile=128064, **kw))
    elif name == "scalar slabs, n 70":
        cs = _case(kernel="K_V2", **dict(_conv(70), tile=128064, **kw))
    elif name == "W 64x320":
        cs = _case(kernel="K_GEMMW", **dict(_conv(320), tile=64320, w_layout=3, **kw))
    elif name == "W 128x160":
        cs = _case(kernel="K_GEMMW", **dict(_conv(160), tile=128160, w_layout=3, slab_rows=8, **kw))
    else:
        d = dict(_conv(160, film=False, resid=False, seed=4))
        acc0 = torch.randn(d["m"], 160, generator=torch.Generator().manual_seed(5))
        d["ref"] = d["ref"] + acc0.double()
        cs = _case(kernel="K_M16", planes=False, inplace=acc0, **dict(d, tile=128160, **kw))
    got = _check(cs, _pitch(out=(12, 4)) if name == "flat in place" else PITCH["a"], f"{name}, ksplit {ksplit}, tickets {tickets}: ")
    assert got.resolved[2] == ksplit
    assert got.resolved[3] == (tickets and name in ("direct, n 160", "flat in place")), "in-launch combine / combine launch: not the expected one"


@pytest.mark.parametrize("lo", [True, False])
@pytest.mark.parametrize("form", ["combine launch, ksplit 2", "combine launch, ksplit 3", "64x80"])
def test_gemm_groupnorm_of_the_result_into_a_wider_plane_buffer(form, lo):
    """gn_*: SiLU(GroupNorm(result)) as planes at column 160 of a 320-wide plane buffer with gn_gamma / gn_beta + 160 (the vectors'
    first 160 entries NaN) - the way the engine's concat-wide buffers are filled -, out_f32 and stat_part as usual."""
    hw, n, cpg = 64, 160, 10
    g = torch.Generator().manual_seed(81)
    gam, bet = torch.randn(n, generator=g) * 0.3 + 1, torch.randn(n, generator=g) * 0.2
    if form == "64x80":
        d = dict(_conv(n, hh=4, ww=16, seed=6), tile=64080, w_layout=3, slab_rows=16)
        kern = "K_GEMMQ"
    else:
        d = dict(_conv(n, seed=6), tile=128160, ksplit=int(form[-1]))
        kern = "K_M16"
    refn = _gn_ref(d["ref"], hw, cpg, gam, bet, 1e-5, 1)
    cs = _case(kernel=kern, stat_cpg=5, lo=lo, gn=dict(gamma=gam, beta=bet, eps=1e-5, silu=1, cpg=cpg), ref_planes=refn, **d)
    _check(cs, _pitch(pl=(160, 160), vec=(160, 160)), f"gn, {form}, out_lo {lo}: ")


# ---- wd_ff_fused
def _ff_pack(w):
    wp = G.split_planes(w).to(DEV)
    wf = torch.empty_like(wp)
    _run("wd_gemm_pack_w", wp[0].data_ptr(), wp[1].data_ptr(), wp.shape[1], wp.shape[2], wf[0].data_ptr(), wf[1].data_ptr(), _st())
    return wf


def _ff_launch(d, P, proj):
    c, m, inner, g = 320, d["m"], d["inner"], P.g
    a = N.WdFfArgs()
    keep, outs = [], []
    xb, xv = G.pitched_planes(d["x"], c + P.src[0], P.src[1], g, DEV)
    a.x_hi, a.x_lo, a.x_ld = xv[0].data_ptr(), xv[1].data_ptr(), xb.shape[-1]
    a.m, a.c, a.inner, a.npass, a.hw_out = m, c, inner, 3, 1
    for nm in ("w1", "w2", "w3"):
        keep.append(_ff_pack(d[nm]))
    vecs = [G.pitched(d[nm][None], d[nm].numel(), 0, g, DEV)[1] for nm in ("b1", "b2", "b3")]
    a.w1_hi, a.w1_lo, a.b1 = keep[0][0].data_ptr(), keep[0][1].data_ptr(), vecs[0].data_ptr()
    a.w2_hi, a.w2_lo, a.b2 = keep[1][0].data_ptr(), keep[1][1].data_ptr(), vecs[1].data_ptr()
    rb, rv = G.pitched(d["res"], c + P.resid[0], P.resid[1], g, DEV)
    a.resid, a.resid_ld = rv.data_ptr(), rb.shape[-1]
    obuf, out = G.guarded(m, c, c + P.out[0], P.out[1], torch.float32, g, DEV)
    pbuf, pl = G.guarded(m, c, c + P.pl[0], P.pl[1], torch.bfloat16, g, DEV, planes=2)
    a.out_f32, a.out_ld = out.data_ptr(), obuf.shape[-1]
    a.out_hi, a.out_lo, a.out_pl_ld = pl[0].data_ptr(), pl[1].data_ptr(), pbuf.shape[-1]
    outs += [("out_f32", obuf, out), ("out planes", pbuf, pl)]
    win = dict(out=out, pl=pl)
    keep += [xb, rb, vecs]
    if proj:
        r3b, r3v = G.pitched(d["res3"], c + P.rowvec[0], P.rowvec[1], g, DEV)
        keep.append(r3b)
        a.w3_hi, a.w3_lo, a.b3 = keep[2][0].data_ptr(), keep[2][1].data_ptr(), vecs[2].data_ptr()
        a.resid3, a.resid3_ld = r3v.data_ptr(), r3b.shape[-1]
        if m % 64 == 0:
            sbuf, part = G.guarded(m // 64, 64, 64, 0, torch.float64, g, DEV)
            a.stat_part, a.stat_cpg, a.hw_out = part.data_ptr(), c // 32, 64
            outs.append(("stat_part", sbuf, part))
            win["stat"] = part
    _run("wd_ff_fused", C.byref(a), _st())
    _sync()
    return types.SimpleNamespace(win=win, outs=outs, keep=keep)


@pytest.mark.parametrize("m", [64, 130])
def test_ff_fused_on_pitched_operands(m):
    """wd_ff_fused, inner = 128: x planes at column 8 of pitch 328, residuals, fp32 and plane outputs padded by 4 / 8 / 12 at
    column 4 - the plain tail, and the w3 (proj_out) tail with its second residual and, at m = 64, the fused statistics."""
    c, inner = 320, 128
    g = torch.Generator().manual_seed(m + inner)
    d = dict(m=m, inner=inner, x=torch.randn(m, c, generator=g))
    w1, b1 = torch.randn(2 * inner, c, generator=g) / c ** 0.5, torch.randn(2 * inner, generator=g)
    w2, w3 = torch.randn(c, inner, generator=g) / inner ** 0.5, torch.randn(c, c, generator=g) / c ** 0.5
    d.update(b2=torch.randn(c, generator=g), b3=torch.randn(c, generator=g), res=torch.randn(m, c, generator=g), res3=torch.randn(m, c, generator=g))
    d.update(w1=geglu_interleave(w1, 16), b1=geglu_interleave(b1, 16), w2=w2, w3=w3)
    xd = d["x"].double()
    hid = (xd @ w1[:inner].double().t() + b1[:inner].double()) * F.gelu(xd @ w1[inner:].double().t() + b1[inner:].double())
    ref = d["res"].double() + hid @ w2.double().t() + d["b2"].double()
    ref3 = d["res3"].double() + ref @ w3.double().t() + d["b3"].double()
    for proj, want in ((False, ref), (True, ref3)):
        dense, got = _ff_launch(d, DENSE, proj), _ff_launch(d, _pitch(src=(8, 8)), proj)
        for name, buf, view in got.outs:
            G.assert_untouched(buf, view, name)
        for key, w in got.win.items():
            G.assert_finite(w, key)
            assert torch.equal(w, dense.win[key]), f"{key}: the pitched launch differs from the dense one"
        e_out, e_pl = rel_err(got.win["out"].cpu(), want), rel_err(_unpl(got.win["pl"]), want)
        print(f"ff m {m} proj {proj}: out {e_out:.3g}, planes {e_pl:.3g}")
        assert e_out < 3e-5 and e_pl < 3e-5
        if "stat" in got.win:
            st, o = got.win["stat"].cpu().reshape(m // 64, 32, 2), want.reshape(m // 64, 64, 32, c // 32)
            assert max_rel(st[..., 0], o.sum(dim=(1, 3))) < 1e-5 and max_rel(st[..., 1], (o * o).sum(dim=(1, 3))) < 1e-5
    assert "stat" in got.win or m % 64


def test_ff_fused_front_on_a_pitched_block_input():
    """The transformer front (x_in): the fp32 block input - also resid3 - at column 4 of pitch 332, its GroupNorm statistics taken
    from that pitched view, out / tok2 / statistics guarded; every other argument is test_gpu_st_fused.py's.  The reference is the
    dense launch of the same kernel (the same bits are asked); what that launch computes is test_gpu_st_fused.py's comparison
    with the three-launch chain, not repeated here."""
    from tests.test_gpu_st_fused import _Block
    blk = _Block(1)
    ref_out, ref_stat, ref_tok2 = blk.fused()
    c, m = blk.c, blk.m
    xb, xv = G.pitched(blk.x.cpu(), 332, 4, 2, DEV)
    gbuf, gpart = G.guarded(blk.B * blk.nchunk, 64, 64, 0, torch.float64, 2, DEV)
    _run("wd_gn_stats", xv.data_ptr(), 332, blk.B, blk.hw, c, c // 32, gpart.data_ptr(), _st())
    obuf, out = G.guarded(m, c, c + 12, 4, torch.float32, 2, DEV)
    tbuf, tok2 = G.guarded(m, c, c, 0, torch.float32, 2, DEV)
    sbuf, stat = G.guarded(blk.B * (blk.hw // 64), 64, 64, 0, torch.float64, 2, DEV)
    f = blk.fused_args(out, stat, tok2)
    f.out_ld = obuf.shape[-1]
    f.x_in, f.x_in_ld, f.gn_part = xv.data_ptr(), 332, gpart.data_ptr()
    f.resid3, f.resid3_ld = xv.data_ptr(), 332
    _run("wd_ff_fused", C.byref(f), _st())
    _sync()
    for name, buf, view in (("out_f32", obuf, out), ("tok2", tbuf, tok2), ("stat_part", sbuf, stat), ("gn_part", gbuf, gpart)):
        G.assert_untouched(buf, view, name)
        G.assert_finite(view, name)
    assert torch.equal(out, ref_out) and torch.equal(tok2, ref_tok2) and torch.equal(stat.reshape(ref_stat.shape), ref_stat)


# ---- the plane producers that feed these GEMMs
def _gn_planes_ref(x, B, hw, ngroups, gam, bet, eps, silu):
    y = F.group_norm(x.double().reshape(B, hw, -1).permute(0, 2, 1), ngroups, gam.double(), bet.double(), eps)
    y = F.silu(y) if silu else y
    return y.permute(0, 2, 1).reshape(x.shape)


@pytest.mark.parametrize("rows,c", [(70, 320), (130, 64)])
def test_layernorm_and_split_on_pitched_operands(rows, c):
    g = torch.Generator().manual_seed(rows + c)
    x = torch.randn(rows, c, generator=g) * 1.5 + 0.3
    gam, bet = torch.randn(c, generator=g) * 0.3 + 1, torch.randn(c, generator=g) * 0.2
    xb, xv = G.pitched(x, c + 12, 4, 2, DEV)
    gv, bv = G.pitched(gam[None], c, 0, 2, DEV)[1], G.pitched(bet[None], c, 0, 2, DEV)[1]
    for what in ("layernorm", "split", "split + SiLU"):
        pbuf, pl = G.guarded(rows, c, c + 24, 8, torch.bfloat16, 2, DEV, planes=2)
        if what == "layernorm":
            _run("wd_layernorm", xv.data_ptr(), xb.shape[-1], rows, c, gv.data_ptr(), bv.data_ptr(), 1e-5, pl[0].data_ptr(), pl[1].data_ptr(),
                 pbuf.shape[-1], _st())
            ref, tol = F.layer_norm(x.double(), (c,), gam.double(), bet.double(), 1e-5), 3e-5
        else:
            silu = what != "split"
            _run("wd_split", xv.data_ptr(), xb.shape[-1], rows, c, int(silu), pl[0].data_ptr(), pl[1].data_ptr(), pbuf.shape[-1], _st())
            ref, tol = (F.silu(x.double()) if silu else x.double()), 1e-5
        _sync()
        G.assert_untouched(pbuf, pl, what)
        G.assert_finite(pl, what)
        e = max_rel(_unpl(pl), ref)
        print(f"{what} {rows} x {c}: max_rel {e:.3g}")
        assert e < tol


@pytest.mark.parametrize("B,hw,c,cpg,part_cpg", [(3, 64, 64, 2, 2), (2, 200, 320, 20, 10)])
def test_groupnorm_producers_on_pitched_operands(B, hw, c, cpg, part_cpg):
    """wd_gn_stats + wd_gn_apply (normalised planes at a column offset of a concat-wide buffer, gamma / beta indexed at c_off +
    channel with NaN in front, raw planes beside them) and wd_gn_apply2 (two sources into one concat-wide buffer)."""
    lib = N.lib()
    g = torch.Generator().manual_seed(B + hw + c)
    m, coff = B * hw, c
    xa, xs = torch.randn(m, c, generator=g) * 1.5 + 0.3, torch.randn(m, c, generator=g) * 0.7 - 0.2
    gam, bet = torch.randn(2 * c, generator=g) * 0.3 + 1, torch.randn(2 * c, generator=g) * 0.2
    nchunk, ngp = lib.wd_gn_nchunk(hw), c // part_cpg
    bufs = {}
    for nm, x in (("a", xa), ("b", xs)):
        xb, xv = G.pitched(x, c + 12, 4, 2, DEV)
        sb, part = G.guarded(B * nchunk, ngp * 2, ngp * 2, 0, torch.float64, 2, DEV)
        _run("wd_gn_stats", xv.data_ptr(), xb.shape[-1], B, hw, c, part_cpg, part.data_ptr(), _st())
        _sync()
        G.assert_untouched(sb, part, "wd_gn_stats part")
        G.assert_finite(part, "wd_gn_stats part")
        st = part.cpu().reshape(B, nchunk, ngp, 2).sum(1)
        o = x.double().reshape(B, hw, ngp, part_cpg)
        assert max_rel(st[..., 0], o.sum(dim=(1, 3))) < 1e-5 and max_rel(st[..., 1], (o * o).sum(dim=(1, 3))) < 1e-5
        bufs[nm] = (xb, xv, part)
    # wd_gn_apply: source b alone, as the second half of the concat (its own groups of cpg channels), + raw planes
    xb, xv, part = bufs["b"]
    gfull, bfull = gam.clone(), bet.clone()
    gfull[:coff] = float("nan")
    bfull[:coff] = float("nan")
    gv, bv = G.pitched(gfull[None], 2 * c, 0, 2, DEV)[1], G.pitched(bfull[None], 2 * c, 0, 2, DEV)[1]
    ld = 2 * c + 16
    pbuf, pl = G.guarded(m, c, ld, 8 + coff, torch.bfloat16, 2, DEV, planes=2)
    rbuf, raw = G.guarded(m, c, ld, 8 + coff, torch.bfloat16, 2, DEV, planes=2)  # (the raw planes share out_ld and c_off)
    base = [t[i].data_ptr() - 2 * coff for t in (pl, raw) for i in range(2)]  # the planes' column 0; the launch writes [c_off, c_off + c)
    _run("wd_gn_apply", xv.data_ptr(), xb.shape[-1], B, hw, c, cpg, part.data_ptr(), nchunk, part_cpg, gv.data_ptr(), bv.data_ptr(), 1e-5, 1,
         base[0], base[1], ld, coff, base[2], base[3], _st())
    _sync()
    for name, buf, view in (("wd_gn_apply planes", pbuf, pl), ("wd_gn_apply raw planes", rbuf, raw)):
        G.assert_untouched(buf, view, name)
        G.assert_finite(view, name)
    ref_b = _gn_planes_ref(xs, B, hw, c // cpg, gam[coff:], bet[coff:], 1e-5, 1)
    e, er = max_rel(_unpl(pl), ref_b), max_rel(_unpl(raw), xs.double())
    print(f"wd_gn_apply: max_rel {e:.3g}, raw {er:.3g}")
    assert e < 3e-5 and er < 1e-5
    # wd_gn_apply2: [a | b] into one concat-wide buffer, raw planes of the concat beside it
    gv, bv = G.pitched(gam[None], 2 * c, 0, 2, DEV)[1], G.pitched(bet[None], 2 * c, 0, 2, DEV)[1]
    pbuf, pl = G.guarded(m, 2 * c, 2 * c + 16, 8, torch.bfloat16, 2, DEV, planes=2)
    rbuf, raw = G.guarded(m, 2 * c, 2 * c + 16, 8, torch.bfloat16, 2, DEV, planes=2)
    (ab, av, pa), (bb, bvw, pb) = bufs["a"], bufs["b"]
    _run("wd_gn_apply2", av.data_ptr(), ab.shape[-1], c, pa.data_ptr(), nchunk, part_cpg, 0, bvw.data_ptr(), bb.shape[-1], c, pb.data_ptr(),
         nchunk, part_cpg, c, B, hw, cpg, gv.data_ptr(), bv.data_ptr(), 1e-5, 1, pl[0].data_ptr(), pl[1].data_ptr(), pbuf.shape[-1],
         raw[0].data_ptr(), raw[1].data_ptr(), None, _st())
    _sync()
    for name, buf, view in (("wd_gn_apply2 planes", pbuf, pl), ("wd_gn_apply2 raw planes", rbuf, raw)):
        G.assert_untouched(buf, view, name)
        G.assert_finite(view, name)
    cat = torch.cat([xa, xs], 1)
    ref2 = _gn_planes_ref(cat, B, hw, 2 * c // cpg, gam, bet, 1e-5, 1)
    e, er = max_rel(_unpl(pl), ref2), max_rel(_unpl(raw), cat.double())
    print(f"wd_gn_apply2: max_rel {e:.3g}, raw {er:.3g}")
    assert e < 3e-5 and er < 1e-5
