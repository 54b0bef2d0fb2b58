"""The training planner's build state: a refused ``plan_train`` call leaves the engine as it found it, and a build that dies
midway leaves nothing behind for the next one.

The plans are built and compared as launch lists - (kernel, what) of every backward op, the bucket cuts and the arena segments -
against a freshly constructed engine on the same model; nothing runs beyond ``refresh_weights`` except in the last test, one
step on the recovered engine whose gradients must equal the fresh engine's bit for bit (the engine sums in fixed orders).
SMALL (64 channels) builds every weight gradient through transposed planes + wd_gemm; FULL at 8 x 32 is there because its
layers wait in the engine's grouped wd_dw queue, the state a dying build used to leave behind."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests._common import FULL, SMALL, make_args  # noqa: E402
from worddiffusion_amd import UNetModel  # noqa: E402
from worddiffusion_amd.synthetic import fill_module_, synthetic_inputs  # noqa: E402

DEV = "cuda:0"
CASES = {"SMALL": (SMALL, (2, 4, 8, 10)), "FULL": (FULL, (2, 8, 32, 10))}  # config, (B, H, W, ctx_len)


def _signature(P):
    return [(fn.__name__, what) for fn, _, what in P.bwd], P.bwd_cuts, P.bwd_segments


@functools.lru_cache(maxsize=None)
def built(cfg_name, die):
    """(engine, plan) of a new model.  die: the first build is killed by a RuntimeError out of the second ``_flush_dw`` call - a host
    exception after the first block's backward was planned, nothing is launched - and the plan is that of the next call."""
    cfg, shape = CASES[cfg_name]
    eng = fill_module_(UNetModel(args=make_args(device=DEV), **cfg), 31).to(DEV).train().train_engine
    eng.refresh_weights()
    if die:
        real, calls = eng._flush_dw, []

        def flush(P):
            calls.append(P)
            if len(calls) == 2:
                raise RuntimeError("the build dies here")
            real(P)

        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(eng, "_flush_dw", flush)
            with pytest.raises(RuntimeError, match="the build dies here"):
                eng.plan_train(*shape)
        assert len(calls) == 2 and not eng._tplans
    return eng, eng.plan_train(*shape)


def test_refused_call_leaves_the_engine_alone():
    eng, P = built("SMALL", False)
    B, H, W, ctx_len = CASES["SMALL"][1]
    with pytest.raises(NotImplementedError):
        eng.plan_train(B, H, W, 0)
    with pytest.raises(ValueError):
        eng.plan_train(B, H, W, ctx_len, 5)  # phoscLabels on the base model
    assert eng.plan_train(B, H, W, ctx_len) is P
    assert len(eng._tplans) == 1


@pytest.mark.parametrize("cfg_name", ["SMALL", "FULL"])
def test_build_that_dies_midway_does_not_leak_into_the_next(cfg_name):
    ops, cuts, segments = _signature(built(cfg_name, True)[1])
    ops_ref, cuts_ref, segments_ref = _signature(built(cfg_name, False)[1])
    assert ops == ops_ref, [(i, a, b) for i, (a, b) in enumerate(zip(ops, ops_ref)) if a != b][:4] + [len(ops), len(ops_ref)]
    assert cuts == cuts_ref and segments == segments_ref


def test_one_step_after_recovery():
    B, H, W, _ = CASES["SMALL"][1]
    inp = synthetic_inputs(B, seed=9, hw=(H, W), num_classes=SMALL["num_classes"])
    dout = torch.randn((B, SMALL["out_channels"], H, W), generator=torch.Generator().manual_seed(4)).to(DEV)
    got = []
    for die in (True, False):
        eng, P = built("SMALL", die)
        out = eng.forward_train(inp["x"].to(DEV), inp["t"].to(DEV), inp["context"].to(DEV), inp["y"].to(DEV))
        assert eng._live is P
        eng.backward(dout, assign=False)
        torch.cuda.synchronize()
        got.append((out.clone(), {k: g.clone() for k, g in eng.grads().items()}))
    (out_a, ga), (out_b, gb) = got
    assert torch.equal(out_a, out_b) and ga and set(ga) == set(gb)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
