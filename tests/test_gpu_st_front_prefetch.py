"""The transformer front of wd_ff_fused requests its operands ahead of the phases that use them (the panel's rows, the proj_in
groups, seven per-channel vectors and b1 staged into LDS in the prologue, Mq a phase early, the chunk-0 weight groups after the
second attention): every moved request against the three-launch chain on the same inputs, and twice against itself - an early
request racing a late reuse of its LDS or registers shows up as a difference between two runs."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests._common import max_rel  # noqa: E402
from tests.test_gpu_st_fused import DEV, _Block  # noqa: E402
from worddiffusion_amd.engine import geglu_interleave  # noqa: E402


class _GemmArgsPatch:
    """The library as _Block.chain() sees it, with the GroupNorm partial geometry of its proj_in launch replaced."""

    def __init__(self, lib, nchunk, pcpg):
        self._lib, self._nchunk, self._pcpg = lib, nchunk, pcpg

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def wd_gemm(self, ref, stream):
        ref._obj.a32_nchunk, ref._obj.a32_pcpg = self._nchunk, self._pcpg
        return self._lib.wd_gemm(ref, stream)


class _FrontBlock(_Block):
    """_Block with every vector the front stages drawn from a seed of its own (a vector staged at another's offset cannot pass),
    and optionally a producer whose partial groups are finer than the consumer's: 5-channel partials in 4 chunks for the
    10-channel groups (gn_cpg / gn_pcpg = 2, gn_nchunk = 4: eight terms per group in the table)."""

    def __init__(self, B, L, ffi, fine):
        super().__init__(B, heads=4, L=L, ffi=ffi)
        c = self.c

        def vec(seed, n=c, sc=0.2, off=0.0):
            return (torch.randn(n, generator=torch.Generator().manual_seed(seed)) * sc + off).to(DEV)

        self.pi_b = vec(101)
        self.n2_g, self.n2_b = vec(102, off=1.0), vec(103)
        self.n3_g, self.n3_b = vec(104, off=1.0), vec(105)
        self.folds = [(q, o, vec(106 + i), rest) for i, (q, o, _, rest) in enumerate(self.folds)]
        self.b1 = geglu_interleave(vec(108, n=2 * ffi, sc=1.0).cpu(), 16).to(DEV)
        self.pcpg = c // 32
        if fine:
            st = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
            p8 = torch.zeros(B, self.nchunk, 64, 2, dtype=torch.float64, device=DEV)
            assert self.nchunk == 8
            assert self.lib.wd_gn_stats(self.x.data_ptr(), c, B, self.hw, c, c // 64, p8.data_ptr(), st) == 0
            self.part = p8.view(B, 4, 2, 64, 2).sum(2).contiguous()
            self.nchunk, self.pcpg = 4, c // 64
            self.lib = _GemmArgsPatch(self.lib, 4, c // 64)

    def fused_args(self, out, stat, tok2):
        f = super().fused_args(out, stat, tok2)
        f.gn_pcpg = self.pcpg
        return f


# (B, L, inner, finer producer partials).  B = 1: four workgroups share one sample's partials; B = 3: the Mq / Mo^T bases differ
# between neighbouring workgroups.  L = 10: HJ = 40, the product shape; L = 3: HJ = 12, one live (head, key) tile, the others take
# the out-of-range descriptor on the early loads.  inner = 1280 (product); 256 and 128: two chunks and one - the chunk-0 groups
# requested from the front next to a short loop, and next to none (the ring runs straight on into proj_out).
CASES = [(1, 10, 1280, False), (3, 10, 1280, False), (3, 3, 1280, False), (1, 3, 256, False), (3, 10, 256, True), (1, 10, 128, True),
         (3, 3, 128, False)]


@pytest.mark.parametrize("B,L,inner,fine", CASES)
def test_front_with_early_requests_equals_the_chain(B, L, inner, fine):
    """Bounds of tests/test_gpu_st_fused.py for this pair of paths: tok2 and output 1e-5 max_rel, statistics 2e-6; a second
    launch on the same inputs gives the same bits."""
    blk = _FrontBlock(B, L, inner, fine)
    ref_out, ref_stat, ref_tok2 = blk.chain()
    out, stat, tok2 = blk.fused()
    assert torch.isfinite(out).all() and torch.isfinite(stat).all() and torch.isfinite(tok2).all()
    e_tok2, e_out, e_stat = max_rel(tok2.cpu(), ref_tok2.cpu()), max_rel(out.cpu(), ref_out.cpu()), max_rel(stat.cpu(), ref_stat.cpu())
    print(f"B={B} L={L} inner={inner} fine={fine}: max_rel tok2 {e_tok2:.3g} out {e_out:.3g} stat {e_stat:.3g}")
    assert e_tok2 <= 1e-5
    assert e_out <= 1e-5
    assert e_stat <= 2e-6
    out2, stat2, tok22 = blk.fused()
    assert torch.equal(out, out2) and torch.equal(stat, stat2) and torch.equal(tok2, tok22)
