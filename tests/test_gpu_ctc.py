"""wd_ctc_loss on the GPU against tests/_ocr_ref.py (itself held to torch's float64 CTC by test_ocr_ref_host.py).

Every operand is a window of a poisoned buffer (tests/_guard.py): logits, dlogits and the int32 targets are pitched windows at an
odd column, the small vectors and the workspace sit between guard runs.  A store outside a window changes the pattern; a read
outside one brings a NaN into an output.

Bars.  Loss and per-sample nll: 1e-5 relative (``check_against_reference``).  Gradient, per sample: the project's
``err < 2e-4 * ||r|| + 1e-7``.  The kernel is also held to torch's own fp32 CTC on the same inputs (computed on the CPU here): its
error may not exceed torch's, or 2^-23 ||r|| + 1e-12 where torch's is below that - the kernel's result is a double rounded once to
fp32, and no fp32 output can be asked to beat its own rounding; where p and the posterior cancel (both ~1) the double difference
itself keeps ~2e-16 per element, 5e-14 over the largest case, hence the absolute term.  Every figure is printed before it is
asserted (profiles/ocr_errors.txt).

Measured on an MI355X (profiles/ocr_errors.txt; worst sample of each case, error of the gradient as a fraction of ||r||, torch's fp32
CTC on the CPU beside it): T256_scale1 2.6e-8 against 8.8e-5, T256_scale8 2.3e-8 against 4.1e-4, T256_scale30 1.7e-8 against 1.5e-3,
T1024 2.5e-8 against 1.9e-3; every case below 4e-8.  Loss and nll within 6e-8 relative on all of them."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _ocr_ref as R  # noqa: E402
from tests._guard import assert_finite, assert_untouched, guarded, guarded_flat  # noqa: E402
from worddiffusion_amd import _native as N  # noqa: E402

DEV = "cuda:0"
BY_NAME = {c["name"]: c for c in R.CASES}
SCALE = 0.375  # (a power-of-two fraction: scale * nll rounds as nll does)


@functools.lru_cache(maxsize=None)
def reference(name):
    c = BY_NAME[name]
    return R.ctc_loss(c["logits"], c["targets"], c["input_len"], c["target_len"], SCALE)


@functools.lru_cache(maxsize=None)
def torch_fp32(name):
    return R.torch_ctc(BY_NAME[name], torch.float32, SCALE)


class Launch:
    """The operands of one call in guarded windows on the device.  ``i64``: the targets as a plain int64 tensor instead."""

    def __init__(self, case, i64=False):
        x, tg = case["logits"], case["targets"]
        self.T, self.B, self.C = x.shape
        self.Lmax = tg.shape[1]
        T, B, C, Lmax = self.T, self.B, self.C, self.Lmax
        self.ld, self.dld, self.tld = C + 13, C + 7, Lmax + 3
        self.bufs = {}

        def window(name, rows, cols, ld, col0, dtype, value=None):
            buf, view = guarded(rows, cols, ld, col0, dtype, device=DEV)
            if value is not None:
                view.copy_(torch.as_tensor(value).reshape(rows, cols))
            self.bufs[name] = (buf, view)
            return view

        def flat(name, n, dtype, value=None):
            buf, view = guarded_flat(n, dtype, device=DEV)
            if value is not None:
                view.copy_(torch.as_tensor(value).reshape(-1))
            self.bufs[name] = (buf, view)
            return view

        self.logits = window("logits", T * B, C, self.ld, 5, torch.float32, x)
        self.dlogits = window("dlogits", T * B, C, self.dld, 3, torch.float32)
        self.i64 = i64
        if i64:
            self.targets = torch.as_tensor(tg).long().to(DEV).contiguous()
            self.tld = Lmax
        else:
            self.targets = window("targets", B, Lmax, self.tld, 1, torch.int32, tg.astype(np.int32))
        self.input_len = flat("input_len", B, torch.int32, case["input_len"])
        self.target_len = flat("target_len", B, torch.int32, case["target_len"])
        self.sample_nll, self.loss = flat("sample_nll", B, torch.float32), flat("loss", 1, torch.float32)
        self.status = flat("status", B, torch.int32)
        self.nbytes = N.lib().wd_ctc_workspace_bytes(T, B, Lmax)
        assert self.nbytes == 8 * B * (1 + T * (5 * Lmax + 3))
        self.work = flat("workspace", self.nbytes // 8, torch.float64)

    def args(self, **over):
        ptr = lambda v: None if v is None else v.data_ptr()  # noqa: E731
        a = dict(logits=ptr(self.logits), ld=self.ld, T=self.T, batch=self.B, C=self.C, targets=ptr(self.targets),
                 targets_i64=int(self.i64), tld=self.tld, Lmax=self.Lmax, input_len=ptr(self.input_len),
                 target_len=ptr(self.target_len), scale=SCALE, dlogits=ptr(self.dlogits), dld=self.dld,
                 sample_nll=ptr(self.sample_nll), loss=ptr(self.loss), status=ptr(self.status), workspace=ptr(self.work),
                 workspace_bytes=self.nbytes)
        a.update(over)
        return list(a.values())

    def run(self, **over):
        rc = N.lib().wd_ctc_loss(*self.args(**over), torch.cuda.current_stream(DEV).cuda_stream)
        torch.cuda.synchronize()
        return rc

    def bits(self, names=("dlogits", "sample_nll", "loss", "status")):
        return {k: self.bufs[k][0].clone().view(torch.int32).cpu() for k in names}

    def all_bits(self):
        return self.bits(tuple(self.bufs))

    def check_guards(self, with_grad=True):
        for name, (buf, view) in self.bufs.items():
            assert_untouched(buf, view, name)
        if with_grad:
            assert_finite(self.dlogits, "dlogits")  # every row t < T is written, the ones past input_len too
        assert_finite(self.loss, "loss")
        assert not bool(torch.isnan(self.sample_nll).any())

    def outputs(self):
        g = self.dlogits.cpu().double().numpy().reshape(self.T, self.B, self.C)
        return g, self.sample_nll.cpu().double().numpy(), float(self.loss.cpu()[0]), self.status.cpu().numpy()


def check_outputs(name, g, nll, loss, ref, against_torch=True):
    """Holds one call's outputs to the bars of the module docstring; prints the figures first."""
    case = BY_NAME[name]
    feasible = np.isfinite(ref["sample_nll"])
    nll_err = float(np.max(np.abs(nll[feasible] - ref["sample_nll"][feasible]) / np.maximum(np.abs(ref["sample_nll"][feasible]), 1e-30),
                           initial=0.0))  # (a reference of exactly 0, one class only, asks for exactly 0)
    loss_err = abs(loss - ref["loss"]) / abs(ref["loss"]) if ref["loss"] else abs(loss)
    rows = []
    for b in range(g.shape[1]):
        err, bar = R.grad_error(g[:, b], ref["dlogits"][:, b])
        rn = float(np.linalg.norm(ref["dlogits"][:, b]))
        terr = R.grad_error(torch_fp32(name)[2][:, b], ref["dlogits"][:, b])[0] if against_torch else float("nan")
        rows.append((b, err, bar, rn, terr))
    worst = max(rows, key=lambda r: r[1] / r[3] if r[3] else 0.0)
    tl = abs(torch_fp32(name)[0] - ref["loss"]) / abs(ref["loss"]) if against_torch and ref["loss"] else float("nan")
    print(f"ocr_errors ctc {name}: loss rel {loss_err:.2e} (torch fp32 {tl:.2e}), nll rel {nll_err:.2e}, worst gradient sample "
          f"{worst[0]}: err {worst[1]:.3e} = {worst[1] / worst[3] if worst[3] else 0.0:.2e} of |r| {worst[3]:.3e}, bar {worst[2]:.3e}, "
          f"torch fp32 err {worst[4]:.3e}")
    assert np.array_equal(np.isinf(nll), ~feasible) and (nll[~feasible] > 0).all(), "an infeasible sample reports nll = +inf"
    assert nll_err <= 1e-5 and loss_err <= 1e-5, (nll_err, loss_err)
    for b, err, bar, rn, terr in rows:
        assert err < bar, (name, b, err, bar)
        if against_torch:
            assert err <= max(terr, 2.0 ** -23 * rn + 1e-12), (name, b, err, terr)
        Tn = int(case["input_len"][b])
        assert not g[Tn:, b].any(), "the gradient is exactly 0 beyond input_len"
        if not feasible[b]:
            assert not g[:, b].any(), "a sample without an alignment has a zero gradient"


# ------------------------------------------------------------------------------------------------------------- G1
@pytest.mark.parametrize("name", R.CASE_IDS)
def test_against_the_specification(name):
    L = Launch(BY_NAME[name])
    assert L.run() == N.WD_OK
    L.check_guards()
    g, nll, loss, status = L.outputs()
    assert not status.any()
    check_outputs(name, g, nll, loss, reference(name))


# ------------------------------------------------------------------------------------------------------------- G2
@pytest.mark.parametrize("name", ["B5_mixed", "T256_scale8"])
def test_loss_only_int64_targets_and_a_second_launch_give_the_same_bits(name):
    L = Launch(BY_NAME[name])
    assert L.run() == N.WD_OK
    first = L.bits()
    L.dlogits.fill_(float("nan"))
    L.sample_nll.fill_(float("nan"))
    L.loss.fill_(float("nan"))
    assert L.run() == N.WD_OK
    second = L.bits()
    for k in first:
        assert torch.equal(first[k], second[k]), f"{k}: the second launch gave other bits"
    # dlogits = NULL: the loss alone, nothing of dlogits touched
    before = L.bits(("dlogits",))["dlogits"]
    L.sample_nll.fill_(float("nan"))
    L.loss.fill_(float("nan"))
    assert L.run(dlogits=None, dld=0) == N.WD_OK
    L.check_guards()
    third = L.bits()
    assert torch.equal(third["dlogits"], before)
    for k in ("sample_nll", "loss", "status"):
        assert torch.equal(first[k], third[k]), f"{k}: loss-only call gave other bits"
    # int64 targets
    M = Launch(BY_NAME[name], i64=True)
    assert M.run() == N.WD_OK
    M.check_guards()
    for a, b in ((L.sample_nll, M.sample_nll), (L.loss, M.loss)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(M.dlogits.view(torch.int32).cpu(), first["dlogits"][2:-2, 3:3 + L.C])


def test_captured_in_a_graph():
    """Two launches and nothing else: the call can be captured, and a replay gives the eager bits."""
    L = Launch(BY_NAME["B5_mixed"])
    assert L.run() == N.WD_OK
    eager = L.bits()
    L.dlogits.fill_(float("nan"))
    L.loss.fill_(float("nan"))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = N.lib().wd_ctc_loss(*L.args(), torch.cuda.current_stream(DEV).cuda_stream)
    assert rc == N.WD_OK
    graph.replay()
    torch.cuda.synchronize()
    replay = L.bits()
    for k in eager:
        assert torch.equal(eager[k], replay[k]), k
    L.check_guards()


# ------------------------------------------------------------------------------------------------------------- G3
BAD_SAMPLES = [  # (sample, field, value, status)
    (1, "id", 51, 4), (1, "id", -1, 4), (1, "id", 1051, 4), (3, "target_len", 10, 2), (3, "target_len", -1, 2),
    (0, "input_len", 0, 1), (0, "input_len", 38, 1), (4, "input_len", -5, 1),
]


@pytest.mark.parametrize("b,field,value,want", BAD_SAMPLES)
def test_a_bad_sample_is_set_aside_and_the_others_keep_their_bits(b, field, value, want):
    """B5_mixed (T = 37, C = 51, Lmax = 9) with one sample's id or length out of range: status names it, its nll and gradient are
    0, every other sample has the bits of the clean call, and the loss is the clean samples' sum."""
    name = "B5_mixed"
    case = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in BY_NAME[name].items()}
    clean = Launch(case)
    assert clean.run() == N.WD_OK
    g0, nll0, _, _ = clean.outputs()
    if field == "id":
        case["targets"][b, 0] = value  # (sample 1 reads one id, target_len[1] = 1)
    else:
        case[field][b] = value
    L = Launch(case)
    assert L.run() == N.WD_OK
    L.check_guards()
    g, nll, loss, status = L.outputs()
    assert list(status) == [want if i == b else 0 for i in range(5)]
    assert nll[b] == 0 and not g[:, b].any()
    others = [i for i in range(5) if i != b]
    assert np.array_equal(g[:, others], g0[:, others]) and np.array_equal(nll[others], nll0[others])
    ref = reference(name)
    keep = np.isfinite(ref["sample_nll"])
    keep[b] = False
    want_loss = SCALE * float(ref["sample_nll"][keep].sum())
    assert abs(loss - want_loss) <= 1e-5 * abs(want_loss), (loss, want_loss)


def test_every_sample_bad():
    case = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in BY_NAME["input_len_short"].items()}
    case["input_len"][:] = [0, 21, -1]
    case["target_len"][1] = 6
    L = Launch(case)
    assert L.run() == N.WD_OK
    L.check_guards()
    g, nll, loss, status = L.outputs()
    assert list(status) == [1, 3, 1] and loss == 0 and not nll.any() and not g.any()


# ------------------------------------------------------------------------------------------------------------- G4
def test_invalid_arguments_launch_nothing():
    L = Launch(BY_NAME["input_len_short"])  # T = 20, B = 3, C = 51, Lmax = 5
    before = L.all_bits()
    D = N.DEFINES
    bad = dict(
        logits_null=dict(logits=None), input_len_null=dict(input_len=None), target_len_null=dict(target_len=None),
        sample_nll_null=dict(sample_nll=None), loss_null=dict(loss=None), status_null=dict(status=None),
        workspace_null=dict(workspace=None), targets_null=dict(targets=None),
        T_0=dict(T=0), T_beyond=dict(T=D["WD_CTC_MAX_T"] + 1), batch_0=dict(batch=0), C_0=dict(C=0),
        C_beyond=dict(C=D["WD_CTC_MAX_C"] + 1, ld=D["WD_CTC_MAX_C"] + 1, dld=D["WD_CTC_MAX_C"] + 1),
        Lmax_negative=dict(Lmax=-1), Lmax_beyond=dict(Lmax=D["WD_CTC_MAX_L"] + 1, tld=D["WD_CTC_MAX_L"] + 1),
        ld_short=dict(ld=50), dld_short=dict(dld=50), tld_short=dict(tld=4), targets_i64_2=dict(targets_i64=2),
        workspace_small=dict(workspace_bytes=L.nbytes - 8), workspace_misaligned=dict(workspace=L.work.data_ptr() + 4),
        logits_misaligned=dict(logits=L.logits.data_ptr() + 2), dlogits_misaligned=dict(dlogits=L.dlogits.data_ptr() + 1),
        targets_i64_misaligned=dict(targets_i64=1, targets=L.targets.data_ptr() + (0 if L.targets.data_ptr() % 8 else 4)),
    )
    for name, over in bad.items():
        assert L.run(**over) == N.WD_EINVAL, name
    after = L.all_bits()
    for name in before:
        assert torch.equal(before[name], after[name]), f"{name} changed although every call was refused"
    assert L.run() == N.WD_OK  # (the operands themselves are fine)
    # with Lmax = 0 (every target empty) the targets may be NULL
    case = dict(BY_NAME["T5_L0"], targets=np.zeros((2, 0), np.int64))
    Z = Launch(case)
    assert Z.Lmax == 0 and Z.run(targets=None) == N.WD_OK
    Z.check_guards()
    g, nll, loss, status = Z.outputs()
    check_outputs("T5_L0", g, nll, loss, reference("T5_L0"), against_torch=False)


# ------------------------------------------------------------------------------------------------------------- G5
def test_optim_ctc_loss():
    """The Python entry point: scale, the flattened target matrix, want_grad=False."""
    from worddiffusion_amd.optim import ctc_loss
    name = "input_len_short"
    c, ref = BY_NAME[name], reference(name)
    x = torch.from_numpy(c["logits"]).to(DEV)
    loss, grad, nll = ctc_loss(x, torch.from_numpy(c["targets"]).reshape(-1), c["input_len"], c["target_len"], scale=SCALE)
    torch.cuda.synchronize()
    check_outputs(name, grad.cpu().double().numpy(), nll.cpu().double().numpy(), float(loss.cpu()[0]), ref, against_torch=False)
    loss2, none, nll2 = ctc_loss(x, torch.from_numpy(c["targets"]), c["input_len"], c["target_len"], want_grad=False, scale=SCALE)
    assert none is None and torch.equal(loss2, loss) and torch.equal(nll2, nll)
