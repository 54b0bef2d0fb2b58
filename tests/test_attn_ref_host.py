"""The host gate of the staircase attention tests (tests/_attn_ref.py, tests/test_gpu_attn_guard.py, tests/test_gpu_xattn_guard.py).
No GPU.

The GPU tests hold the kernels to the suite's tolerances (fp32 result 2e-5, planes 3e-5, max_rel against fp64) on inputs whose
logits span 29 to more than 60 nats.  That is only a fair demand if the kernels' arithmetic class - split-bf16 operands, fp32
scores, exp2 - stays well inside the tolerance on exactly those inputs, so for every staircase case the GPU tests run:
  * the host emulation of the class is within 1e-5 of fp64 (half the GPU tolerance).  A case that does not meet this is replaced,
    never given a wider bound;
  * the case has teeth: the same emulation with the rescale factor alpha forced to 1 after the first block - the bug the staircase
    exists for - is off by more than 100 x 2e-5.  A descending staircase cannot show that bug (its maximum never moves: asserted, the
    forced variant gives the same bits); what it shows in the key-split form is the merge of two key groups with different maxima,
    so there the merge factors forced to 1 must be off by as much."""
import pytest
import torch

from tests import _attn_ref as R

GATE = 1e-5          # emulation vs fp64: half of the GPU tolerance
TEETH = 100 * 2e-5   # the forced-alpha variant vs fp64


def _id(cs):
    return "-".join(f"{v:.3g}" if isinstance(v, float) else str(int(v)) for v in cs)


@pytest.mark.parametrize("cs", R.STAIRCASE, ids=_id)
def test_staircase_case_is_within_the_arithmetic_class_and_has_teeth(cs):
    B, H, nq, nk, d, scale, step, period, desc = cs
    q, k, v, off = R.staircase(B, H, nq, nk, d, scale, step, period, desc)
    ref = R.attention_fp64(q, k, v, B, H, nq, nk, d, scale)
    span = R.span_nats(q, k, B, H, nq, nk, d, scale)
    st = {}
    emu = R.emulate_mfma(q, k, v, B, H, nq, nk, d, scale, stats=st)
    e_mfma, e_f32 = R.max_rel(emu, ref), R.max_rel(R.emulate_fp32(q, k, v, B, H, nq, nk, d, scale), ref)
    bad = R.emulate_mfma(q, k, v, B, H, nq, nk, d, scale, force_alpha_one=True)
    e_bad = R.max_rel(bad, ref)
    print(f"span {span:.1f} nats, emulation {e_mfma:.2e}, fp32 class {e_f32:.2e}, live rescales {st['rescales']}, "
          f"largest exp2 argument {st['max_exp2']:.2f}, alpha forced to 1: {e_bad:.2e}")
    assert span > 25.0 and float(off.max()) > 20.0
    assert e_mfma <= GATE
    if cs in R.GENERIC_STAIRCASE:   # attn_kernel runs these through WDIFF_ATTN_GENERIC: the fp32 class has to meet the gate too
        assert e_f32 <= GATE
    assert -1e29 < st["max_exp2"] <= R.FA_LAZY
    if not desc:
        assert st["rescales"] > 0 and e_bad > TEETH
        if step * R.LOG2E < R.FA_LAZY:
            assert st["max_exp2"] > 1.0   # exponentials above 2: the maximum was exceeded inside the headroom
    else:
        assert st["rescales"] == 0 and torch.equal(bad, emu)
        if nq <= 64:
            e_merge = R.max_rel(R.emulate_mfma(q, k, v, B, H, nq, nk, d, scale, force_merge_one=True), ref)
            print(f"merge factors forced to 1: {e_merge:.2e}")
            assert e_merge > TEETH


@pytest.mark.parametrize("cs", R.SMALL_STAIRCASE, ids=_id)
def test_small_kernel_staircase_is_within_the_fp32_class(cs):
    """attn_small_kernel keeps its nk scores in registers and subtracts their maximum once - no running state, so no alpha; a stair
    of 7 nats at every key spans 63 (nk = 10) and 105 (nk = 16) nats, and the teeth are the subtraction itself: without it
    exp(105) is not an fp32 number."""
    B, H, nq, nk, d, scale, desc = cs
    q, k, v, off = R.staircase(B, H, nq, nk, d, scale, 7, 1, desc)
    ref = R.attention_fp64(q, k, v, B, H, nq, nk, d, scale)
    err = R.max_rel(R.emulate_fp32(q, k, v, B, H, nq, nk, d, scale), ref)
    print(f"span {R.span_nats(q, k, B, H, nq, nk, d, scale):.1f} nats, fp32 class {err:.2e}")
    assert float(off.max()) > 60.0 and err <= GATE
    if nk == 16:
        s = R.logits_fp64(q, k, B, H, nq, nk, d, scale).float()
        assert not bool(torch.isfinite(torch.exp(s)).all())


@pytest.mark.parametrize("cs", R.XATTN_STAIRCASE, ids=_id)
def test_folded_cross_attention_staircase_is_within_the_arithmetic_class(cs):
    """The stairs are put into K before the fold; the MFMA form multiplies the split-bf16 planes of the folded matrices, so the
    gate is on that class.  (One softmax over L <= 40 keys in registers: no running state here either.)"""
    B, hw, c, heads, L, step, period = cs
    o = R.xattn_operands(B, hw, c, heads, L, step=step, period=period)
    mq, _, ref, _ = R.xattn_fp64(o, B, hw, c, heads, L)
    n1 = R._layer_norm(o["x"].double(), o["ga"].double(), o["be"].double(), 1e-5).view(B, hw, c)
    s = torch.einsum("btn,bkn->btk", n1, mq).view(B, hw, heads, L)
    span = float((s.max(-1).values - s.min(-1).values).max())
    err = R.max_rel(R.emulate_xattn16(o, B, hw, c, heads, L), ref)
    print(f"span {span:.1f} nats, emulation {err:.2e}")
    assert span > step * ((L - 1) // period) - 3.0 and err <= GATE


def test_the_emulation_is_the_plain_attention_on_plain_inputs():
    """On 0.5 * randn operands (the inputs of tests/test_gpu_kernels.py) both forms meet the same gate,
    the key-split form with an idle second group (nk <= 32) included, and forcing alpha to 1 changes nothing: the rescale fires once,
    on an empty accumulator - which is why those inputs cannot see a wrong rescale."""
    g = torch.Generator().manual_seed(5)
    for B, H, nq, nk, d in ((2, 2, 40, 17, 32), (1, 2, 100, 96, 48), (1, 1, 33, 200, 16)):
        q, k, v = (torch.randn(B * n, H * d, generator=g) * 0.5 for n in (nq, nk, nk))
        ref = R.attention_fp64(q, k, v, B, H, nq, nk, d, 0.3)
        st = {}
        emu = R.emulate_mfma(q, k, v, B, H, nq, nk, d, 0.3, stats=st)
        assert R.max_rel(emu, ref) <= GATE and st["rescales"] == 0
        assert torch.equal(emu, R.emulate_mfma(q, k, v, B, H, nq, nk, d, 0.3, force_alpha_one=True))
        assert R.max_rel(R.emulate_mfma(q, k, v, B, H, nq, nk, d, 0.3, ksplit=nq > 64), ref) <= GATE
