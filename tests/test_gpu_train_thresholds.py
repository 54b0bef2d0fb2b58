"""Training gradients on both sides of every batch size at which the training step's launch plan changes (FULL config, 8 x 32
latents, 10 context tokens; phosc: plus the 769-int PHOSC vector), through the reference's call surface: model -> MSELoss ->
backward, eager, so that ``TrainEngine.plan_train`` is the planner under test.

The training plan depends on the batch far more than the forward's: ``_dw_form`` chooses per layer between ``wd_dw``, a grouped
``wd_dw_group`` launch and transposed planes + ``wd_gemm``, the library picks the token slicing of both ``wd_dw`` forms from M, every
data-gradient GEMM picks tile and K cut from its grid, and ``_stage_dout`` hands out private or shared scratch by those forms.  So
the plan of B differs from that of B - 1 at nearly every B: THRESHOLDS is not derived here, tools/plan_thresholds.py scanned
B = 1..72 (train-base) and 1..32 (train-phosc) into profiles/plan_thresholds_train_<variant>.txt, and
tests/test_plan_thresholds_host.py holds the tables below to those files.  The kernels are tested one by one elsewhere
(test_gpu_dw_guard.py, test_gpu_backward_guard.py, test_gpu_pitch.py); what is tested here is the training planner handing them
the right operands at b - 1 and at b.

Reference: ``RunningReference`` (tests/_train_ref.py) - the float64 oracle under autograd on the CPU, folded in sample by sample over
one pool of distinct samples per variant, so that the cases in ascending B cost one pass over the pool together
(tests/test_train_running_ref_host.py holds it to the batched construction).  A case uses the first B samples.  The bars are those
of ``check_against_reference``, unchanged: per-sample prediction max_rel < 5e-5, loss 1e-5 relative, the same set of parameters
with a gradient, per parameter ||g - ref|| < 2e-4 ||ref|| + 1e-7; between two batch sizes a sample's prediction max_rel < 5e-5."""
import os
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests._common import FULL, max_rel  # noqa: E402
from tests._plan_sig import diff, read_scan, release, train_signature_at  # noqa: E402
from tests._train_ref import DEV, RunningReference, check_against_reference, train_call, train_model  # noqa: E402
from worddiffusion_amd.synthetic import synthetic_inputs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHOSC_LEN = 769
SEED_W = 0

# the B column of profiles/plan_thresholds_train_<variant>.txt (scan of B = 1..72 / 1..32)
THRESHOLDS = {
    "base": tuple(range(2, 69)) + (70, 71),
    "phosc": tuple(range(2, 33)),
}
SCANNED_TO = {"base": 72, "phosc": 32}                   # the top of each scan: the largest case, and the size of the pool
POOL_SEEDS = {"base": (13, 14), "phosc": (15, 16)}       # seeds of synthetic_inputs and of eps
TEETH_SHARE = 0.95


def batch_sizes(variant) -> tuple:
    """b - 1 and b of every threshold and the scan's upper end, ascending; neighbours that coincide once."""
    return tuple(sorted({B for b in THRESHOLDS[variant] for B in (b - 1, b)} | {SCANNED_TO[variant]}))


GRADIENT_CASES = [(v, B) for v in THRESHOLDS for B in batch_sizes(v)]
THRESHOLD_CASES = [(v, b) for v in THRESHOLDS for b in THRESHOLDS[v]]


def scan_file(variant) -> str:
    return os.path.join(ROOT, "profiles", f"plan_thresholds_train_{variant}.txt")


def pool_inputs(variant):
    n, (seed_in, seed_eps) = SCANNED_TO[variant], POOL_SEEDS[variant]
    inp = synthetic_inputs(n, seed_in, phosc_len=PHOSC_LEN if variant == "phosc" else 0)
    eps = torch.from_numpy(np.random.RandomState(seed_eps).standard_normal(tuple(inp["x"].shape)).astype(np.float32))
    # every sample is its own: a kernel that read a neighbour's row, timestep, word or writer would not get away with it
    assert len({inp["x"][b].numpy().tobytes() for b in range(n)}) == n
    assert len({eps[b].numpy().tobytes() for b in range(n)}) == n
    for k in ("t", "context", "y"):
        assert len({inp[k][b].numpy().tobytes() for b in range(n)}) > n // 2, k
    return inp, eps


class _Pools:
    """Per variant, made on first use and kept for the module: the model on the device in train mode, the pool's inputs and eps,
    the running float64 reference (``ref=True``: the plan test never asks for it) with the CPU seconds it has cost, and the
    predictions of the steps already run (B -> CPU tensor), which the cross-threshold test reads again."""

    def __init__(self):
        self._v = {}

    def get(self, variant, ref=False):
        if variant not in self._v:
            inp, eps = pool_inputs(variant)
            self._v[variant] = dict(model=train_model(FULL, variant, variant == "phosc", SEED_W), inp=inp, eps=eps, outs={}, ref_s=0.0)
        pool = self._v[variant]
        if ref and "ref" not in pool:
            pool["ref"] = RunningReference(FULL, variant, pool["inp"], pool["eps"], PHOSC_LEN if variant == "phosc" else 0, seed_w=SEED_W)
        return pool


@pytest.fixture(scope="module")
def pools():
    p = _Pools()
    yield p
    for v in p._v.values():
        release(v["model"].train_engine)


def train_step(pool, variant, B, twice=False):
    """``train_call`` of the model on the first B samples of the pool -> (pred, loss, {name: grad}) on the CPU.  twice: a second
    call after zero_grad returns the same gradient bits.  Gradients are dropped and the plan is released afterwards."""
    m, inp = pool["model"], {k: v[:B] for k, v in pool["inp"].items()}
    phosc_len = PHOSC_LEN if variant == "phosc" else 0
    try:
        pred, loss, grads = train_call(m, variant, inp["x"], inp, pool["eps"][:B], phosc_len)
        pred, grads = pred.detach().cpu(), {k: g.detach().cpu().clone() for k, g in grads.items()}
        if twice:
            m.zero_grad(set_to_none=True)
            pred2, loss2, again = train_call(m, variant, inp["x"], inp, pool["eps"][:B], phosc_len)
            assert torch.equal(pred2.detach().cpu(), pred) and loss2 == loss, "a second call returned another prediction or loss"
            assert set(again) == set(grads)
            moved = [k for k, g in grads.items() if not torch.equal(again[k].detach().cpu(), g)]
            assert not moved, f"a second call after zero_grad changed the bits of {len(moved)} gradients: {moved[:8]}"
        return pred, loss, grads
    finally:
        m.zero_grad(set_to_none=True)
        release(m.train_engine)


@pytest.mark.parametrize("variant", list(THRESHOLDS))
def test_every_listed_threshold_changes_the_train_plan(pools, variant):
    """Plans only: the training plan of b differs from that of b - 1 exactly as the scan file says, and between two listed batch
    sizes nothing changes (the plan of b_i is the plan of b_(i+1) - 1; that of the last threshold the plan of the scan's end)."""
    eng = pools.get(variant)["model"].train_engine
    want = read_scan(scan_file(variant))
    phosc_len = PHOSC_LEN if variant == "phosc" else 0
    sig = {B: train_signature_at(eng, B, phosc_len) for B in batch_sizes(variant)}
    for b in THRESHOLDS[variant]:
        assert sig[b - 1] != sig[b], f"B = {b}: the plan is that of B = {b - 1}"
        assert diff(sig[b - 1], sig[b]) == want[b], f"B = {b}"
    for b, nxt in zip(THRESHOLDS[variant], THRESHOLDS[variant][1:] + (SCANNED_TO[variant] + 1,)):
        assert sig[b] == sig[nxt - 1], f"a threshold between B = {b} and B = {nxt - 1}: {diff(sig[b], sig[nxt - 1])}"


@pytest.mark.parametrize("variant,B", GRADIENT_CASES, ids=[f"{v}-{B}" for v, B in GRADIENT_CASES])
def test_training_gradients_on_both_sides_of_a_threshold(pools, variant, B):
    """Prediction, loss and every parameter gradient of the first B samples against the float64 reference; at a threshold b (not at
    b - 1) a second step after zero_grad returns the same bits.

    Teeth: whenever the reference advanced by exactly one sample, the share of parameters (reference norm > 1e-6) at which the
    reference WITHOUT that sample's contribution misses the gradient bar is printed; at the largest B of each variant it must be
    at least 95 %.  Measured (profiles/train_thresholds_errors.txt): 205 of 205 parameters at base B = 72 and 213 of 213 at phosc
    B = 32, and 100 % at every smaller B but base B = 24 (181 of 205) and base B = 53 (182 of 205) - one sample of 72 moves a
    gradient by about 1 / B of its norm, far more than the bar's 2e-4."""
    pool = pools.get(variant, ref=True)
    pred, loss, grads = train_step(pool, variant, B, twice=B in THRESHOLDS[variant])
    pool["outs"][B] = pred
    assert pred.shape == (B, 4, 8, 32) and pred.dtype == torch.float32 and torch.isfinite(pred).all()
    t0 = time.time()
    ref = pool["ref"].at(B)
    share = pool["ref"].drop_one_share()
    pool["ref_s"] += time.time() - t0
    print()
    if share is not None:
        print(f"[train thresholds] {variant} B = {B}: sample {B - 1} left out of the reference misses the gradient bar at {share[0]} of "
              f"{share[1]} parameters ({100.0 * share[0] / share[1]:.1f} %)")
    if B == SCANNED_TO[variant]:
        print(f"[train thresholds] float64 running reference, {variant}: {B} samples in {pool['ref_s']:.1f} s of CPU")
        assert share is not None, "the largest case did not advance the reference by one sample: run the cases in ascending B"
        assert share[0] >= TEETH_SHARE * share[1], f"the gradient bar has no teeth at B = {B}: {share}"
    check_against_reference(pred, loss, grads, ref, f"[train thresholds] {variant} B = {B}")


@pytest.mark.parametrize("variant,b", THRESHOLD_CASES, ids=[f"{v}-{b}" for v, b in THRESHOLD_CASES])
def test_a_sample_keeps_its_prediction_across_a_threshold(pools, variant, b):
    """The first b - 1 samples' predictions of the B = b step against the B = b - 1 step: when a case above fails, this says which
    side moved."""
    pool = pools.get(variant)
    lo, hi = (pool["outs"][B] if B in pool["outs"] else train_step(pool, variant, B)[0] for B in (b - 1, b))
    errs = [max_rel(hi[i], lo[i]) for i in range(b - 1)]
    worst = max(range(b - 1), key=errs.__getitem__)
    print(f"\n[train thresholds] {variant} B = {b - 1} -> {b}: worst sample {worst}, max_rel {errs[worst]:.3e} between the two steps")
    assert errs[worst] < 5e-5, [(i, e) for i, e in enumerate(errs) if e >= 5e-5]
