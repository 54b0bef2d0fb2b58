"""The GEGLU block of wd_ff_kernel (csrc/wd_ff.hip): the first product leaves its accumulators transposed (a lane's four registers
are four hidden units of ONE token), the block evaluates them two at a time and stores eight bytes per plane and row tile into
the h image the second product reads.  A second weight that PICKS hidden units makes every element of that image visible:

    w2[n, (7 n) % 384] = 1, zero elsewhere, b2 = 0, resid = 0    =>    out[:, n] = hidden unit (7 n) % 384 of every token

(7 is coprime to 384: the 320 picked units are distinct and lie in all three chunks, all eight waves and every lq), so a unit
written to the wrong token or K position is wrong by O(1).  c = 320, inner = 384, m = 64 and 70 (a ragged panel); the plain
tail in three passes and in one, and the folded proj_out tail (W3 = I: W32 = W3 W2 is the pick matrix itself, b32 = 0).

Placement bound: max_rel against fp64 (x W1x^T + b1x) . gelu(x W1g^T + b1g), at most TWICE what the parent of the change that
transposed the block measured on the same inputs, and never above test_fused_geglu_feed_forward's 3e-5 / 3e-2.  Measured on
MI355X (max over m = 64, 70):

    tail, passes      parent      this tree
    plain, 3          5.757e-06   5.757e-06
    plain, 1          5.508e-03   5.508e-03
    folded, 3         5.757e-06   5.757e-06

Gate sweep: every W1 row zero, b1x = 1, b1g = 384 gates over [-8, 8] with +-0, +-1e-6, +-1e-3 and +-3.135 (where the error of
the erf formula peaks) among the picked ones, so out = gelu(gate).  |out - ref| <= 2^-16 |ref| + 6e-7 max(1, |g|): the first
term is the split-bf16 plane pair h goes through, the second the formula in fp32 (Abramowitz & Stegun 7.1.26 with a reciprocal
one ulp off either way: <= 4.6e-7 absolute and <= 3.8e-7 |g| against fp64 over 200 001 gates of [-8, 8] on the CPU), with about
1.5 x left for v_exp_f32.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests._common import max_rel  # noqa: E402
from tests.test_gpu_kernels import DEV, _st, planes_of  # noqa: E402
from worddiffusion_amd import _native as N  # noqa: E402
from worddiffusion_amd.engine import geglu_interleave  # noqa: E402

FC, INNER = 320, 384
PICK = [(7 * n) % INNER for n in range(FC)]
# (npass, folded) -> max_rel of the parent's library on these inputs (the table above)
PARENT = {(3, False): 5.757e-06, (1, False): 5.508e-03, (3, True): 5.757e-06}
CAP = {3: 3e-5, 1: 3e-2}


def _pack(lib, w):
    wp = planes_of(w.to(DEV))
    wf = torch.empty_like(wp)
    N.check(lib.wd_gemm_pack_w(wp[0].data_ptr(), wp[1].data_ptr(), wp.shape[1], wp.shape[2], wf[0].data_ptr(), wf[1].data_ptr(), _st()),
            "wd_gemm_pack_w")
    return wf


class _Case:
    """One launch of wd_ff_fused with the pick matrix as second weight; `out` is NaN-filled before every launch."""

    def __init__(self, m, npass, fold, x, w1, b1):
        self.lib = lib = N.lib()
        assert lib.wd_ff_supported(FC, INNER)
        pick = torch.zeros(FC, INNER)
        pick[torch.arange(FC), torch.tensor(PICK)] = 1.0
        self.keep = keep = [_pack(lib, geglu_interleave(w1, 16)), _pack(lib, pick), geglu_interleave(b1, 16).to(DEV), planes_of(x.to(DEV)),
                            torch.zeros(m, FC, device=DEV), torch.zeros(FC, device=DEV)]
        w1f, w2f, b1d, xp, zres, zb = keep
        self.out = torch.empty(m, FC, device=DEV)
        a = self.a = N.WdFfArgs()
        a.x_hi, a.x_lo, a.x_ld = xp[0].data_ptr(), xp[1].data_ptr(), FC
        a.m, a.c, a.inner = m, FC, INNER
        a.w1_hi, a.w1_lo, a.b1 = w1f[0].data_ptr(), w1f[1].data_ptr(), b1d.data_ptr()
        a.w2_hi, a.w2_lo, a.b2 = w2f[0].data_ptr(), w2f[1].data_ptr(), zb.data_ptr()
        a.resid, a.resid_ld = zres.data_ptr(), FC
        a.out_f32, a.out_ld = self.out.data_ptr(), FC
        a.hw_out, a.npass = 1, npass
        if fold:  # out = x_in + h (W3 W2)^T + tok2 W3^T + b32 with W3 = I, tok2 = resid = 0, no x_in: W32 is the pick matrix
            keep.append(_pack(lib, torch.eye(FC)))
            a.w3_hi, a.w3_lo, a.b3 = keep[-1][0].data_ptr(), keep[-1][1].data_ptr(), zb.data_ptr()
            a.w32_hi, a.w32_lo, a.b32 = w2f[0].data_ptr(), w2f[1].data_ptr(), zb.data_ptr()

    def run(self):
        self.out.fill_(float("nan"))
        N.check(self.lib.wd_ff_fused(C.byref(self.a), _st()), "wd_ff_fused")
        torch.cuda.synchronize()
        return self.out.clone()


def _placement_inputs(m):
    g = torch.Generator().manual_seed(1000 + m)
    x = torch.randn(m, FC, generator=g)
    w1 = torch.randn(2 * INNER, FC, generator=g) / FC ** 0.5
    b1 = torch.randn(2 * INNER, generator=g)
    xd, wd = x.double(), w1.double()
    hid = (xd @ wd[:INNER].t() + b1[:INNER].double()) * F.gelu(xd @ wd[INNER:].t() + b1[INNER:].double())
    return x, w1, b1, hid[:, PICK]


_INPUTS = {}


def _inputs(m):
    if m not in _INPUTS:
        _INPUTS[m] = _placement_inputs(m)
    return _INPUTS[m]


@pytest.mark.parametrize("npass,fold", [(3, False), (1, False), (3, True)])
@pytest.mark.parametrize("m", [64, 70])
def test_geglu_block_puts_every_hidden_unit_in_its_place(m, npass, fold):
    x, w1, b1, ref = _inputs(m)
    out = _Case(m, npass, fold, x, w1, b1).run().cpu()
    err = max_rel(out, ref)
    bound = min(2.0 * PARENT[(npass, fold)], CAP[npass])
    print(f"m={m} npass={npass} fold={fold}: max_rel {err:.3e} (bound {bound:.3e}, parent {PARENT[(npass, fold)]:.3e}) lib {N.LIB_PATH}")
    assert torch.isfinite(out).all()
    assert err <= bound


def _gates():
    g = torch.linspace(-8.0, 8.0, INNER)
    special = [0.0, -0.0, 1e-6, -1e-6, 1e-3, -1e-3, 3.135, -3.135, 8.0, -8.0]
    for k, v in enumerate(special):
        g[PICK[31 * k]] = v  # picked units, spread over the chunks and waves
    return g


@pytest.mark.parametrize("fold", [False, True])
def test_geglu_gate_sweep(fold):
    m = 70
    gates = _gates()
    b1 = torch.cat([torch.ones(INNER), gates])
    x = torch.randn(m, FC, generator=torch.Generator().manual_seed(5))
    out = _Case(m, 3, fold, x, torch.zeros(2 * INNER, FC), b1).run().cpu().double()
    gp = gates[PICK]
    ref = F.gelu(gp.double())
    assert bool(torch.isin(torch.tensor([1e-6, -1e-6, 1e-3, -1e-3, 3.135, -3.135]), gp).all())  # the special gates are picked ones
    assert int((gp == 0).sum()) == 2 and int(torch.signbit(gp[gp == 0]).sum()) == 1
    tol = 2.0 ** -16 * ref.abs() + 6e-7 * gp.double().abs().clamp(min=1.0)
    diff = (out - ref).abs()
    worst = int((diff / tol).max(dim=0).values.argmax())
    print(f"fold={fold}: largest |out - ref| / tol {float((diff / tol).max()):.3f} at gate {float(gp[worst]):.6g}; "
          f"max |out - ref| {float(diff.max()):.3e} lib {N.LIB_PATH}")
    assert torch.isfinite(out).all()
    assert bool((diff <= tol).all())
    assert torch.equal(out, out[:1].expand_as(out))  # every token row holds the same values


@pytest.mark.parametrize("npass,fold", [(3, False), (3, True), (1, False)])
def test_geglu_block_repeats_bit_for_bit(npass, fold):
    x, w1, b1, _ = _inputs(70)
    case = _Case(70, npass, fold, x, w1, b1)
    first = case.run()
    assert torch.equal(first, case.run())
