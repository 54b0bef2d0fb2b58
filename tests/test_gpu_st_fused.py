"""The base-model SpatialTransformer of the 8 x 32 level as one wd_ff_fused launch (wd_ff_args.x_in, the transformer front):
against the three-launch chain it replaces - wd_gemm (GroupNorm applied while staging + proj_in) -> wd_xattn_pair (both folded
cross-attentions + norm3 planes) -> wd_ff_fused (feed-forward + proj_out + next GroupNorm statistics) - on the same inputs, and
the engine's plan with WDIFF_FUSE_ST on and off."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests._common import FULL, make_args, max_rel  # noqa: E402
from worddiffusion_amd import UNetModel, UNetModelPhosc  # noqa: E402
from worddiffusion_amd import _native as N  # noqa: E402
from worddiffusion_amd.engine import geglu_interleave  # noqa: E402
from worddiffusion_amd.synthetic import fill_module_, synthetic_inputs  # noqa: E402

DEV = "cuda:0"


def _st():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _planes(x):
    hi = x.to(torch.bfloat16)
    return torch.stack([hi, (x - hi.float()).to(torch.bfloat16)], 0).contiguous()


def _pack(lib, w):
    wp = _planes(w.to(DEV))
    wf = torch.empty_like(wp)
    N.check(lib.wd_gemm_pack_w(wp[0].data_ptr(), wp[1].data_ptr(), wp.shape[1], wp.shape[2], wf[0].data_ptr(), wf[1].data_ptr(), _st()),
            "wd_gemm_pack_w")
    return wf


class _Block:
    """Seeded parameters and inputs of one transformer (c = inner = 320, one block) at B x 8 x 32, and both ways to run it."""

    def __init__(self, B, heads=4, L=10, ffi=1280, seed=0):
        lib = self.lib = N.lib()
        g = torch.Generator().manual_seed(seed + B)
        c, hw = 320, 256
        d = c // heads
        self.B, self.c, self.hw, self.m, self.heads, self.L, self.ffi = B, c, hw, B * hw, heads, L, ffi
        r = lambda *s, sc=1.0, off=0.0: (torch.randn(*s, generator=g) * sc + off).to(DEV)  # noqa: E731
        self.x = r(self.m, c, sc=1.5, off=0.3)
        self.gn_g, self.gn_b = r(c, sc=0.3, off=1.0), r(c, sc=0.2)
        self.pi_w, self.pi_b = _pack(lib, torch.randn(c, c, generator=g) / c ** 0.5), r(c, sc=0.1)
        self.n2_g, self.n2_b = r(c, sc=0.2, off=1.0), r(c, sc=0.2)
        self.n3_g, self.n3_b = r(c, sc=0.2, off=1.0), r(c, sc=0.2)
        self.folds = []
        for _ in range(2):
            k, v = r(B * L, c), r(B * L, c)
            wq, wo = r(c, c, sc=c ** -0.5), r(c, c, sc=c ** -0.5)
            mq, mo = torch.zeros(B, heads * L, c, device=DEV), torch.zeros(B, heads * L, c, device=DEV)
            mq_pl = torch.zeros(B, 2, 64, c, dtype=torch.bfloat16, device=DEV)
            mot_pl = torch.zeros(B, 2, c, 64, dtype=torch.bfloat16, device=DEV)
            N.check(lib.wd_xattn_fold(k.data_ptr(), c, v.data_ptr(), c, B, heads, L, d, float(d ** -0.5), wq.data_ptr(), wo.data_ptr(),
                                      c, mq.data_ptr(), mo.data_ptr(), mq_pl.data_ptr(), mot_pl.data_ptr(), _st()), "fold")
            self.folds.append((mq_pl, mot_pl, r(c, sc=0.1), (k, v, wq, wo, mq, mo)))
        w1 = torch.randn(2 * ffi, c, generator=g) / c ** 0.5
        self.w1, self.b1 = _pack(lib, geglu_interleave(w1, 16)), geglu_interleave(torch.randn(2 * ffi, generator=g), 16).to(DEV)
        self.w2, self.b2 = _pack(lib, torch.randn(c, ffi, generator=g) / ffi ** 0.5), r(c, sc=0.1)
        self.w3, self.b3 = _pack(lib, torch.randn(c, c, generator=g) / c ** 0.5), r(c, sc=0.1)
        self.nchunk = lib.wd_gn_nchunk(hw)
        self.part = torch.zeros(B, self.nchunk, 32, 2, dtype=torch.float64, device=DEV)
        N.check(lib.wd_gn_stats(self.x.data_ptr(), c, B, hw, c, c // 32, self.part.data_ptr(), _st()), "stats")

    def ff_args(self, out, stat):
        a = N.WdFfArgs()
        a.m, a.c, a.inner, a.npass = self.m, self.c, self.ffi, 3
        a.w1_hi, a.w1_lo, a.b1 = self.w1[0].data_ptr(), self.w1[1].data_ptr(), self.b1.data_ptr()
        a.w2_hi, a.w2_lo, a.b2 = self.w2[0].data_ptr(), self.w2[1].data_ptr(), self.b2.data_ptr()
        a.w3_hi, a.w3_lo, a.b3 = self.w3[0].data_ptr(), self.w3[1].data_ptr(), self.b3.data_ptr()
        a.resid3, a.resid3_ld = self.x.data_ptr(), self.c
        a.out_f32, a.out_ld = out.data_ptr(), self.c
        a.stat_part, a.stat_cpg, a.hw_out = stat.data_ptr(), self.c // 32, self.hw
        return a

    def chain(self):
        lib, c, m = self.lib, self.c, self.m
        a = N.WdGemmArgs()
        s0 = N.WdSrc()
        s0.ld, s0.c, s0.ntaps, s0.hw_src = c, c, 1, self.hw
        a.src[0], a.nsrc, a.npass = s0, 1, 3
        a.w_hi, a.w_lo, a.w_layout, a.tile, a.ksplit = self.pi_w[0].data_ptr(), self.pi_w[1].data_ptr(), 3, 64320, 1
        a.m, a.n, a.ktot, a.hw_out = m, c, c, self.hw
        a.bias = self.pi_b.data_ptr()
        tok = torch.full((m, c), float("nan"), device=DEV)
        a.out_f32, a.out_ld = tok.data_ptr(), c
        a.a32, a.a32_ld, a.a32_part = self.x.data_ptr(), c, self.part.data_ptr()
        a.a32_nchunk, a.a32_pcpg, a.a32_cpg = self.nchunk, c // 32, c // 32
        a.a32_gamma, a.a32_beta, a.a32_eps, a.a32_silu = self.gn_g.data_ptr(), self.gn_b.data_ptr(), 1e-6, 0
        N.check(lib.wd_gemm(C.byref(a), _st()), "proj_in")
        tok2 = torch.full((m, c), float("nan"), device=DEV)
        n3 = torch.zeros(2, m, c, dtype=torch.bfloat16, device=DEV)
        (qa, oa, ba, _), (qb, ob, bb, _) = self.folds
        g2, b2 = self.n2_g.data_ptr(), self.n2_b.data_ptr()
        N.check(lib.wd_xattn_pair(tok.data_ptr(), c, self.B, self.hw, c, 1e-5, self.heads, self.L, g2, b2, qa.data_ptr(), oa.data_ptr(),
                                  ba.data_ptr(), g2, b2, qb.data_ptr(), ob.data_ptr(), bb.data_ptr(), tok2.data_ptr(), c,
                                  self.n3_g.data_ptr(), self.n3_b.data_ptr(), 1e-5, n3[0].data_ptr(), n3[1].data_ptr(), c, _st()), "pair")
        out = torch.full((m, c), float("nan"), device=DEV)
        stat = torch.full((self.B, self.hw // 64, 32, 2), float("nan"), dtype=torch.float64, device=DEV)
        f = self.ff_args(out, stat)
        f.x_hi, f.x_lo, f.x_ld = n3[0].data_ptr(), n3[1].data_ptr(), c
        f.resid, f.resid_ld = tok2.data_ptr(), c
        N.check(lib.wd_ff_fused(C.byref(f), _st()), "ff + proj_out")
        torch.cuda.synchronize()
        return out, stat, tok2

    def fused_args(self, out, stat, tok2):
        c = self.c
        f = self.ff_args(out, stat)
        f.x_in, f.x_in_ld, f.hw = self.x.data_ptr(), c, self.hw
        f.gn_part, f.gn_nchunk, f.gn_pcpg, f.gn_cpg, f.gn_eps = self.part.data_ptr(), self.nchunk, c // 32, c // 32, 1e-6
        f.gn_gamma, f.gn_beta = self.gn_g.data_ptr(), self.gn_b.data_ptr()
        f.pi_hi, f.pi_lo, f.pi_b = self.pi_w[0].data_ptr(), self.pi_w[1].data_ptr(), self.pi_b.data_ptr()
        f.ln2_gamma, f.ln2_beta, f.ln3_gamma, f.ln3_beta, f.ln_eps = (self.n2_g.data_ptr(), self.n2_b.data_ptr(), self.n3_g.data_ptr(),
                                                                      self.n3_b.data_ptr(), 1e-5)
        (qa, oa, ba, _), (qb, ob, bb, _) = self.folds
        f.mq_a, f.mot_a, f.xb_a = qa.data_ptr(), oa.data_ptr(), ba.data_ptr()
        f.mq_b, f.mot_b, f.xb_b = qb.data_ptr(), ob.data_ptr(), bb.data_ptr()
        f.heads, f.L, f.tok2 = self.heads, self.L, tok2.data_ptr()
        return f

    def fused(self):
        out = torch.full((self.m, self.c), float("nan"), device=DEV)
        stat = torch.full((self.B, self.hw // 64, 32, 2), float("nan"), dtype=torch.float64, device=DEV)
        tok2 = torch.full((self.m, self.c), float("nan"), device=DEV)
        f = self.fused_args(out, stat, tok2)
        N.check(self.lib.wd_ff_fused(C.byref(f), _st()), "transformer (fused)")
        torch.cuda.synchronize()
        return out, stat, tok2


@pytest.mark.parametrize("B", [4, 64])
def test_fused_transformer_launch_equals_the_chain(B):
    """wd_ff_fused with the transformer front == wd_gemm (a32 proj_in) -> wd_xattn_pair -> wd_ff_fused (proj_out), the same
    operations on the same operands: output, next-GroupNorm statistics and the tok2 residual agree to max_rel 1e-5 (measured:
    up to 3.3e-6 - last-bit differences of the fp32 LayerNorm / softmax code as compiled into the two kernels, amplified by the
    peaked softmax of these random folds; not bit-identical); a second launch gives the same bits."""
    _fused_equals_the_chain(_Block(B))


def _fused_equals_the_chain(blk):
    B = blk.B
    ref_out, ref_stat, ref_tok2 = blk.chain()
    out, stat, tok2 = blk.fused()
    assert torch.isfinite(out).all() and torch.isfinite(stat).all()
    assert max_rel(tok2.cpu(), ref_tok2.cpu()) <= 1e-5
    assert max_rel(out.cpu(), ref_out.cpu()) <= 1e-5
    assert max_rel(stat.cpu(), ref_stat.cpu()) <= 2e-6
    print(f"B={B} heads={blk.heads} L={blk.L}: out bit-identical {torch.equal(out, ref_out)}, stat_part bit-identical "
          f"{torch.equal(stat, ref_stat)}, max_rel out {max_rel(out.cpu(), ref_out.cpu()):.3g}")
    out2, stat2, tok22 = blk.fused()
    assert torch.equal(out, out2) and torch.equal(stat, stat2) and torch.equal(tok2, tok22)


@pytest.mark.parametrize("heads,L", [(1, 10), (2, 10), (8, 5)])
def test_fused_transformer_launch_equals_the_chain_at_other_head_counts(heads, L):
    """The same comparison with d = 320 / 160 / 40 (--num_heads 1 / 2 / 8; eight heads fold with at most 5 keys: heads * L <= 40), at
    the smallest m of the test above.  (The fold these launches read is held to fp64 at these head counts by
    test_gpu_kernels.py::test_folded_cross_attention.)"""
    _fused_equals_the_chain(_Block(4, heads=heads, L=L))


def test_fused_transformer_refuses_what_it_does_not_cover():
    blk = _Block(4)
    out = torch.empty(blk.m, blk.c, device=DEV)
    stat = torch.empty(blk.B, blk.hw // 64, 32, 2, dtype=torch.float64, device=DEV)
    tok2 = torch.empty(blk.m, blk.c, device=DEV)
    lib = blk.lib

    def refused(**kw):
        f = blk.fused_args(out, stat, tok2)
        for k, v in kw.items():
            setattr(f, k, v)
        return lib.wd_ff_fused(C.byref(f), _st()) == N.WD_EINVAL

    assert refused(hw=100)               # a panel would straddle samples
    assert refused(m=blk.m - 64)         # m not a whole number of samples
    assert refused(npass=1)
    assert refused(w3_hi=None)           # the front only comes with the proj_out tail
    assert refused(L=11)                 # heads * L > 40
    assert refused(mq_b=None)
    assert refused(gn_part=None)
    assert refused(tok2=None)
    assert refused(gn_cpg=7)             # groups must divide the channels and be whole partials


def _build(variant, phosc_on, seed=0):
    cls = UNetModel if variant == "base" else UNetModelPhosc
    m = cls(args=make_args(device=DEV, phosc=1 if phosc_on else 0), **FULL)
    fill_module_(m, seed)
    return m.to(DEV).eval()


def _steps(m):
    P = next(iter(m.engine._plans.values()))
    return [what for _, _, what in P.step]


def test_engine_fused_transformer_switch(monkeypatch):
    """FULL base model at B = 64: WDIFF_FUSE_ST=1 (default) and 0 give the same forward (max_rel 2e-5; measured 7.1e-6), the fused plan has 6
    launches fewer (three transformers at 8 x 32, three launches -> one each); the PHOSC plan does not change."""
    inp = synthetic_inputs(64, seed=5)
    outs, steps = [], []
    for on in ("0", "1"):
        monkeypatch.setenv("WDIFF_FUSE_ST", on)
        m = _build("base", False, seed=2)
        assert m.engine.fuse_st == (on == "1")
        with torch.no_grad():
            outs.append(m(inp["x"].to(DEV), None, original_images=None, timesteps=inp["t"].to(DEV), context=inp["context"].to(DEV),
                          y=inp["y"].to(DEV)))
        steps.append(_steps(m))
        del m
    assert torch.isfinite(outs[1]).all()
    assert max_rel(outs[1].cpu(), outs[0].cpu()) <= 2e-5
    print(f"fused vs chain: bit-identical {torch.equal(outs[0], outs[1])}, max_rel {max_rel(outs[1].cpu(), outs[0].cpu()):.3g}")
    assert len(steps[0]) - len(steps[1]) == 6
    assert sum(1 for w in steps[1] if "proj_in + a1 + a2" in w) == 3
    inp = synthetic_inputs(64, seed=6, phosc_len=769)
    pst = []
    for on in ("0", "1"):
        monkeypatch.setenv("WDIFF_FUSE_ST", on)
        m = _build("phosc", True, seed=2)
        with torch.no_grad():
            m(inp["x"].to(DEV), inp["phosc"].to(DEV), timesteps=inp["t"].to(DEV), context=inp["context"].to(DEV), y=inp["y"].to(DEV))
        pst.append(_steps(m))
        del m
    assert pst[0] == pst[1]
