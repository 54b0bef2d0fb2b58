"""Writer dropout in the captured training step (``TrainStep(label_dropout=p)``), held to the host specification of
``tests/_labeldrop_ref.py``:

  1. ``label_dropout=0`` is the step without the argument: the same launch list, the same loss and gradients bit for bit;
  2. ``label_dropout=0.5``: a replayed graph draws the next rows (device-read row base), the second call meets the float64 oracle
     carrying the specification's mask at its own rows, a fresh ``TrainStep`` with the same seed reproduces the first call;
  3. ``accumulate=2`` at B = 3 draws the mask of one B = 6 call and accumulates its gradient;
  4. together with ``dropout=0.1`` the oracle carries both host masks.

Bounds: those of ``tests/test_gpu_dropout.check_against_reference`` (prediction 5e-5, loss 1e-5, every gradient within
2e-4 ||ref|| + 1e-7)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet_oracle as U  # noqa: E402
from tests import _labeldrop_ref as R  # noqa: E402
from tests._common import FULL, SMALL, make_args  # noqa: E402
from tests.test_gpu_dropout import (P_DROP, case_inputs, check_against_reference, dropped_resblock, oracle_layers,  # noqa: E402
                                    train_model)
from worddiffusion_amd import Diffusion, UNetModel  # noqa: E402
from worddiffusion_amd.optim import FusedAdamW  # noqa: E402
from worddiffusion_amd.synthetic import fill_module_, synthetic_inputs, synthetic_tensor  # noqa: E402
from worddiffusion_amd.training import TrainStep  # noqa: E402

DEV = "cuda:0"
SEEDS, HW = (21, 203, 4), (8, 16)
P_LABEL = 0.5


def reference64(B, keep, drop=None):
    """float64 oracle (x_t = noise_images(x0, t, eps)) with the writer term where ``keep`` holds -> MSE -> autograd:
    (pred, loss, {name: grad}).  drop = (seed, row_base): the ResBlocks carry the host dropout mask of ``tests/_dropout_ref.py``
    as well."""
    x, inp, eps = case_inputs(B, HW, SEEDS, noised=True)
    sd = {k: torch.from_numpy(synthetic_tensor(k, s, SEEDS[0])).double().requires_grad_(True)
          for k, s in U.state_dict_shapes(FULL, "base")}
    orc = R.KeepOracle(FULL, sd, "base", False)
    orc.keep = np.asarray(keep, dtype=bool)
    with pytest.MonkeyPatch.context() as mp:
        if drop is not None:
            mp.setattr(U, "resblock", dropped_resblock(oracle_layers("base"), drop[0], drop[1], P_DROP))
        pred = orc(x.double(), inp["t"], inp["context"], inp["y"], None)
    loss = torch.nn.functional.mse_loss(pred, eps.double())
    loss.backward()
    return pred.detach(), float(loss.detach()), {k: v.grad for k, v in sd.items() if v.grad is not None}


def _diff():
    return Diffusion(noise_steps=1000, img_size=(64, 256), args=make_args(device=DEV))


def _run(step, x0, inp, eps, rows=slice(None)):
    loss = float(step(x0[rows].to(DEV), inp["context"][rows].to(DEV), inp["y"][rows].to(DEV), t=inp["t"][rows],
                      noise=eps[rows].to(DEV)).cpu())
    torch.cuda.synchronize()
    return step._P.out.cpu(), loss, {k: g.clone() for k, g in step.eng.grads().items()}


def _ops(P):
    return [(fn.__name__, what) for fn, _, what in list(P.step) + list(P.bwd)]


# ------------------------------------------------------------------------------------------ 1. p = 0
def test_label_dropout_zero_is_the_step_without_the_argument():
    inp = synthetic_inputs(4, seed=9, hw=(4, 8), num_classes=SMALL["num_classes"])
    eps = torch.randn(inp["x"].shape, generator=torch.Generator().manual_seed(4))
    got = []
    for kw in ({}, dict(label_dropout=0.0)):
        m = fill_module_(UNetModel(args=make_args(device=DEV), **SMALL), 31).to(DEV).train()
        step = TrainStep(m, Diffusion(noise_steps=1000, img_size=(32, 64), args=make_args(device=DEV)),
                         FusedAdamW(m.parameters(), lr=1e-3), seed=5, **kw)
        calls = [_run(step, inp["x"], inp, eps) for _ in range(2)]
        got.append((calls, _ops(step._P), list(m.train_engine._tplans)))
        with pytest.raises(RuntimeError, match="label_dropout"):
            step.last_writer_keep
    (a, ops_a, keys_a), (b, ops_b, keys_b) = got
    assert ops_a == ops_b and keys_a == keys_b
    assert not any(name == "wd_label_rows_keep" for name, _ in ops_b)
    for (pa, la, ga), (pb, lb, gb) in zip(a, b):
        assert la == lb and torch.equal(pa, pb) and set(ga) == set(gb)
        for k in ga:
            assert torch.equal(ga[k], gb[k]), k
    assert a[0][1] != a[1][1]  # lr > 0: the second call is a different step, and still the same in both


# ------------------------------------------------------------------------------------------ 2. the draw, replayed
def test_train_step_draws_the_next_rows_on_every_replay():
    B = 3
    seed, _, _, p = R.DRAWS["step call 0"]
    assert p == P_LABEL
    masks = [R.keep_mask(*R.DRAWS[k]) for k in ("step call 0", "step call 1")]
    assert not np.array_equal(masks[0], masks[1])
    x0, inp, eps = case_inputs(B, HW, SEEDS)
    m = train_model("base", SEEDS[0], dropout=0)
    opt = FusedAdamW(m.parameters(), lr=0.0)
    step = TrainStep(m, _diff(), opt, seed=seed, use_graph=True, label_dropout=p)
    first = _run(step, x0, inp, eps)
    keep0 = step.last_writer_keep.cpu().clone()
    second = _run(step, x0, inp, eps)
    keep1 = step.last_writer_keep.cpu().clone()
    assert step._graph is not None
    assert keep0.tolist() == masks[0].astype(int).tolist() and keep1.tolist() == masks[1].astype(int).tolist()
    assert sum(name == "wd_label_rows_keep" for name, _ in _ops(step._P)) == 1
    check_against_reference(*second, reference64(B, masks[1]), f"TrainStep label_dropout {p}, call 1 (rows {B}..), mask {keep1.tolist()}")
    lab = second[2]["label_emb.weight"].cpu()
    kept_rows = sorted(set(inp["y"][torch.from_numpy(masks[1])].tolist()))
    others = torch.ones(lab.shape[0], dtype=torch.bool)
    others[kept_rows] = False
    assert not bool(lab[others].view(torch.int32).any()) and all(bool(lab[r].any()) for r in kept_rows)
    assert not torch.equal(first[0], second[0])
    again = _run(TrainStep(m, _diff(), opt, seed=seed, use_graph=True, label_dropout=p), x0, inp, eps)
    assert again[1] == first[1] and torch.equal(again[0], first[0]) and set(again[2]) == set(first[2])
    for k, g in first[2].items():
        assert torch.equal(again[2][k], g), f"{k}: a fresh TrainStep with the same seed gave another gradient"
    # eager launches draw what the graph draws
    eager = _run(TrainStep(m, _diff(), opt, seed=seed, use_graph=False, label_dropout=p), x0, inp, eps)
    assert torch.equal(eager[0], first[0])


# ------------------------------------------------------------------------------------------ 3. accumulation
def test_two_calls_of_3_draw_and_accumulate_what_one_call_of_6_does():
    seed, _, _, p = R.DRAWS["step B=6"]
    mask6 = R.keep_mask(*R.DRAWS["step B=6"])
    x0, inp, eps = case_inputs(6, HW, SEEDS)
    m = train_model("base", SEEDS[0], dropout=0)
    big = TrainStep(m, _diff(), FusedAdamW(m.parameters(), lr=0.0), seed=seed, label_dropout=p)
    whole = _run(big, x0, inp, eps)
    assert big.last_writer_keep.cpu().tolist() == mask6.astype(int).tolist()
    m2 = train_model("base", SEEDS[0], dropout=0)
    acc = TrainStep(m2, _diff(), FusedAdamW(m2.parameters(), lr=0.0), seed=seed, accumulate=2, label_dropout=p)
    halves = []
    for a in range(2):
        halves.append(_run(acc, x0, inp, eps, slice(3 * a, 3 * a + 3)))
        assert acc.last_writer_keep.cpu().tolist() == mask6[3 * a:3 * a + 3].astype(int).tolist(), a
    assert (acc.micro_index, acc.optimizer_steps, acc.step_index) == (0, 1, 2)
    got, ref = halves[1][2], whole[2]
    assert set(got) == set(ref)
    bad = []
    for k, r in ref.items():
        err, rn = float((got[k].double() - r.double()).norm()), float(r.double().norm())
        if not err < 2e-4 * rn + 1e-7:
            bad.append((k, err, rn))
    assert not bad, bad[:8]
    mean = 0.5 * (halves[0][1] + halves[1][1])
    assert abs(mean - whole[1]) <= 1e-5 * abs(whole[1])


# ------------------------------------------------------------------------------------------ 4. with the ResBlock dropout
def test_label_dropout_is_orthogonal_to_the_resblock_dropout():
    B = 3
    seed, row_base, _, p = R.DRAWS["step call 0"]
    mask = R.keep_mask(*R.DRAWS["step call 0"])
    x0, inp, eps = case_inputs(B, HW, SEEDS)
    m = train_model("base", SEEDS[0], dropout=P_DROP)
    step = TrainStep(m, _diff(), FusedAdamW(m.parameters(), lr=0.0), seed=seed, label_dropout=p)
    got = _run(step, x0, inp, eps)
    assert step.last_writer_keep.cpu().tolist() == mask.astype(int).tolist()
    names = [name for name, _ in _ops(step._P)]
    assert names.count("wd_label_rows_keep") == 1 and names.count("wd_gn_apply_dropout") == len(step._P.dropouts) - 1 > 0
    check_against_reference(*got, reference64(B, mask, drop=(seed, row_base)),
                            f"TrainStep label_dropout {p} + dropout {P_DROP}, mask {mask.astype(int).tolist()}")
