"""tests/_ocr_ref.py, the float64 specification of the CTC loss, against torch.nn.functional.ctc_loss in float64 on the shared case
table: loss, per-sample nll and the gradient with respect to the raw logits.  Both sides are float64 and differ only in the order
of their sums, so the bars are a few thousand ulp of the quantities compared, not an accuracy budget.  No GPU.

One row per sample is torch's own and not the derivative: when the LAST target id equals the blank, torch's backward
initialises the last step's row by assignment, state 2L first and state 2L - 1 second, so the second (also class 0) overwrites the
first instead of adding to it; the row's posteriors then no longer sum to 1 and the log-softmax backward spreads the difference
over the whole row.  The specification keeps the sum (the formula of include/wdiff_hip.h), and for exactly that row, input_len - 1
of such a sample, the test holds it to central differences of the specification's own nll instead."""
import numpy as np
import pytest
import torch

from tests import _ocr_ref as R


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_specification_against_torch_float64(case):
    scale = 0.375
    ref = R.ctc_loss(case["logits"], case["targets"], case["input_len"], case["target_len"], scale)
    assert not ref["status"].any(), "the case table holds valid samples only"
    loss, nll, grad = R.torch_ctc(case, torch.float64, scale)
    feasible = np.isfinite(ref["sample_nll"])
    assert np.array_equal(nll[~feasible], np.zeros((~feasible).sum())), "torch reports an infeasible sample as 0 (zero_infinity)"
    assert np.allclose(ref["sample_nll"][feasible], nll[feasible], rtol=1e-11, atol=1e-11)
    assert abs(ref["loss"] - loss) <= 1e-11 * abs(loss) + 1e-12
    assert ref["dlogits"].shape == grad.shape
    for b in range(grad.shape[1]):
        Tn, L = int(case["input_len"][b]), int(case["target_len"][b])
        if feasible[b] and L > 0 and case["targets"][b, L - 1] == 0:  # (see the module docstring)
            x = case["logits"].astype(np.float64)
            nll_at = lambda d: R.ctc_sample(x[:Tn, b] + d, case["targets"][b, :L])[0]  # noqa: E731
            for c in range(x.shape[2]):
                d = np.zeros((Tn, x.shape[2]))
                d[Tn - 1, c] = 1e-5
                fd = scale * (nll_at(d) - nll_at(-d)) / 2e-5
                assert abs(ref["dlogits"][Tn - 1, b, c] - fd) <= 1e-8, (b, c, ref["dlogits"][Tn - 1, b, c], fd, grad[Tn - 1, b, c])
            grad[Tn - 1, b] = ref["dlogits"][Tn - 1, b]
        err = float(np.linalg.norm(ref["dlogits"][:, b] - grad[:, b]))
        assert err <= 1e-10 * float(np.linalg.norm(grad[:, b])) + 1e-13, (b, err)
        assert not ref["dlogits"][int(case["input_len"][b]):, b].any()
        if not feasible[b]:
            assert not ref["dlogits"][:, b].any()


def test_the_table_covers_what_it_is_meant_to():
    by = {c["name"]: c for c in R.CASES}
    nll = lambda n: R.ctc_loss(*(by[n][k] for k in ("logits", "targets", "input_len", "target_len")))["sample_nll"]  # noqa: E731
    assert np.isfinite(nll("repeat_exact")).all()
    assert list(np.isfinite(nll("repeat_one_short"))) == [False, True]  # 'aab' in three steps has no alignment, 'abc' has one
    assert {2 * int(c["target_len"].max()) + 1 for c in R.CASES} >= {1, 3, 63, 65, 85, 129, 255}  # both sides of 64, 128 states
    assert {c["logits"].shape[2] for c in R.CASES} >= {1, 51, 54, 256}
    assert {c["logits"].shape[0] for c in R.CASES} >= {1, 5, 256, 1024}
    assert any((c["targets"][0, :int(c["target_len"][0])] == 0).any() for c in R.CASES)
    assert any((c["input_len"] < c["logits"].shape[0]).any() for c in R.CASES)


def test_status_word():
    ids = np.array([3, 50, 0, 51, -1])
    assert R.check_sample(51, 8, 5, ids, 8, 3) == 0
    assert R.check_sample(51, 8, 5, ids, 0, 3) == 1 and R.check_sample(51, 8, 5, ids, 9, 3) == 1
    assert R.check_sample(51, 8, 5, ids, 8, 6) == 2 and R.check_sample(51, 8, 5, ids, 8, -1) == 2
    assert R.check_sample(51, 8, 5, ids, 8, 4) == 4 and R.check_sample(51, 8, 5, ids, 9, 5) == 5
    x = np.random.RandomState(0).standard_normal((8, 2, 51))
    out = R.ctc_loss(x, np.stack([ids, np.array([1, 2, 3, 4, 5])]), [8, 8], [4, 5])
    assert list(out["status"]) == [4, 0] and out["sample_nll"][0] == 0 and not out["dlogits"][:, 0].any()
    alone = R.ctc_loss(x[:, 1:], np.array([[1, 2, 3, 4, 5]]), [8], [5])
    assert out["loss"] == alone["loss"] and np.array_equal(out["dlogits"][:, 1], alone["dlogits"][:, 0])


def test_greedy_decode_specification():
    T, C = 9, 5
    path = [0, 2, 2, 0, 2, 3, 3, 0, 1]
    x = np.full((T, 1, C), -1.0)
    x[np.arange(T), 0, path] = 1.0
    assert R.greedy_decode(x) == [[2, 2, 3, 1]]
