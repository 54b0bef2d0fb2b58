"""Host gate of ``RunningReference`` (tests/_train_ref.py), the additive float64 reference of tests/test_gpu_train_thresholds.py: on the
SMALL config (base, and phosc with 21 PHOSC ints), 4 x 8 latents and a pool of 5 samples, the running sum of per-sample gradients
is the one batched float64 ``mse_loss`` backward of ``reference64``, whatever order it is asked in, and leaving one sample out of
it is caught by the gradient bar of ``check_against_reference``.  No GPU: the oracle runs on the CPU."""
import numpy as np
import pytest
import torch

from tests._common import SMALL
from tests._train_ref import RunningReference, batched_reference64, check_against_reference, misses_the_gradient_bar
from worddiffusion_amd.synthetic import synthetic_inputs

HW, POOL_N, SEEDS = (4, 8), 5, (3, 21, 8)  # seeds: weights, inputs, eps
CASES = {"base": 0, "phosc": 21}            # variant -> phosc_len


def _pool(variant):
    inp = synthetic_inputs(POOL_N, seed=SEEDS[1], hw=HW, num_classes=SMALL["num_classes"], phosc_len=CASES[variant])
    eps = torch.from_numpy(np.random.RandomState(SEEDS[2]).standard_normal(tuple(inp["x"].shape)).astype(np.float32))
    return inp, eps


def _running(variant):
    inp, eps = _pool(variant)
    return RunningReference(SMALL, variant, inp, eps, CASES[variant], seed_w=SEEDS[0])


def _batched(variant, B):
    inp, eps = _pool(variant)
    head = {k: v[:B] for k, v in inp.items()}
    return batched_reference64(SMALL, variant, head["x"], head, eps[:B], CASES[variant], SEEDS[0])


def _same(got, want, label):
    """1e-12 relative per parameter with norm > 1e-6 and 1e-14 absolute otherwise; loss and predictions to 1e-12."""
    (pred, loss, grads), (pred_w, loss_w, grads_w) = got, want
    assert pred.shape == pred_w.shape and pred.dtype == torch.float64
    assert float((pred - pred_w).abs().max()) <= 1e-12 * float(pred_w.abs().max()), label
    assert abs(loss - loss_w) <= 1e-12 * abs(loss_w), (label, loss, loss_w)
    assert set(grads) == set(grads_w), label
    worst = 0.0
    for k, r in grads_w.items():
        err, rn = float((grads[k] - r).norm()), float(r.norm())
        if rn > 1e-6:
            worst = max(worst, err / rn)
            assert err <= 1e-12 * rn, (label, k, err, rn)
        else:
            assert float((grads[k] - r).abs().max()) <= 1e-14, (label, k)
    return worst


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request):
    """(variant, the running reference asked for 2, 3 and 5 in ascending order, its three answers)."""
    run = _running(request.param)
    answers = {}
    for B in (2, 3, 5):
        answers[B] = run.at(B)
        assert run.count == B
    return request.param, run, answers


@pytest.mark.parametrize("B", [2, 3, 5])
def test_the_running_sum_is_the_batched_backward(case, B):
    variant, _, answers = case
    worst = _same(answers[B], _batched(variant, B), f"{variant} at({B})")
    print(f"\n[running reference] SMALL {variant} at({B}): worst relative difference to the batched backward {worst:.1e}")


def test_a_lower_batch_starts_over(case, capsys):
    """``at(3)`` after ``at(5)`` is ``at(3)`` of a fresh reference - the restart path - and says that it started over."""
    variant, run, _ = case
    assert run.at(5)[1] > 0 and run.count == 5
    capsys.readouterr()
    again = run.at(3)
    assert "starting over" in capsys.readouterr().out and run.count == 3
    fresh = _running(variant).at(3)
    _same(again, fresh, f"{variant} at(3) after at(5)")
    _same(again, _batched(variant, 3), f"{variant} at(3) after at(5), batched")
    assert run.drop_one_share() is None  # (that advance folded three samples in)


def test_leaving_the_last_sample_out_is_caught(case):
    """Teeth: (G_5 - g_4) / (5 n), the reference of the five samples without the last one's contribution, misses the gradient bar of
    ``check_against_reference`` at EVERY parameter whose reference norm exceeds 1e-6."""
    variant, run, _ = case
    run.at(4)
    pred, loss, ref = run.at(5)
    lo, hi, g_last = run.last
    assert (lo, hi) == (4, 5)
    scale = 1.0 / (5 * run.n)
    dropped = {k: (run.G[k] - g_last[k]) * scale for k in ref}
    asked = [k for k, r in ref.items() if float(r.norm()) > 1e-6]
    under = [k for k in asked if not misses_the_gradient_bar(dropped[k], ref[k])]
    rels = [float((dropped[k] - ref[k]).norm() / ref[k].norm()) for k in asked]
    print(f"\n[running reference] SMALL {variant}: sample 4 left out of 5: smallest relative error {min(rels):.2g} against the bar of "
          f"2e-4, {len(under)} of {len(asked)} parameters under the bar")
    assert len(asked) > 100 and not under, under[:8]
    assert run.drop_one_share() == (len(asked), len(asked))
    with pytest.raises(AssertionError, match="gradients off the reference"):
        check_against_reference(pred, loss, dropped, (pred, loss, ref), f"SMALL {variant} without sample 4")
    check_against_reference(pred, loss, ref, (pred, loss, ref), f"SMALL {variant}")  # (the bar itself passes what is right)
