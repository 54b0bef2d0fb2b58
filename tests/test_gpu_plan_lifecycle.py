"""Plan life cycles: what a training script does to ONE model between building a plan and dropping it - batch sizes that alternate,
forwards between a forward and its backward, a ``TrainStep`` that shares its model - and the inference engine's LRU plan cache.
SMALL base model, latents 4 x 8, 10 context tokens, B in {1, 2, 3}.

The reference of every sequence is a FRESH model (and engine) that made only the call under test on the same inputs, compared with
``torch.equal``.  That needs the path to be bit-reproducible between two fresh models, which ``test_fresh_models_agree_bit_for_bit``
establishes first, one assertion per path (training call, eval forward, both samplers, ``TrainStep`` captured and eager): the
engines sum in fixed orders and use no float atomics, so all of them are, and no sequence here falls back to the oracle's bars.
"Equal to fresh" is anchored to the mathematics once: ``test_shapes_that_come_back`` also holds its result to the float64 oracle at
the unchanged bars of ``check_against_reference``.

What is refused (DESIGN.md "Plan life cycles"): the backward of a training forward whose intermediates a later training forward
overwrote (same shape) or whose plan it released (another shape) raises a RuntimeError before any ``param.grad`` is touched."""
import collections
import copy
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests._common import SMALL, make_args  # noqa: E402
from tests._train_ref import DEV, case_inputs, check_against_reference, reference64, train_call, train_model  # noqa: E402
from worddiffusion_amd import Diffusion, UNetModel  # noqa: E402
from worddiffusion_amd import _native as N  # noqa: E402
from worddiffusion_amd import engine as E  # noqa: E402
from worddiffusion_amd.optim import FusedAdamW  # noqa: E402
from worddiffusion_amd.synthetic import fill_module_, synthetic_inputs  # noqa: E402
from worddiffusion_amd.training import TrainStep  # noqa: E402

CFG, VAR, HW, IMG, L = SMALL, "base", (4, 8), (32, 64), 10
SEEDS = (0, 2, 5)  # weights, inputs, eps
T = 6              # noise steps of the sampler calls: "a few steps"
STALE = "a later forward on this model overwrote the activations this backward needs"
mse = torch.nn.MSELoss()


# ------------------------------------------------------------------------------------------ training: helpers
def case(B, k=0):
    """(x, inputs, eps) of batch B; k > 0: other inputs of the same shape."""
    return case_inputs(CFG, B, HW, 0, (SEEDS[0], SEEDS[1] + 10 * k, SEEDS[2] + 10 * k))


def fresh():
    return train_model(CFG, VAR, False, SEEDS[0])


def fwd(m, c):
    x, inp, _ = c
    return m(x.to(DEV), timesteps=inp["t"].to(DEV), context=inp["context"].to(DEV), y=inp["y"].to(DEV))


def loss_of(c, pred):
    return mse(c[2].to(DEV), pred)


def grads_of(m):
    torch.cuda.synchronize()
    return {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}


def run(m, c):
    """train_call with results that survive the next call (``param.grad`` are views of the engine's gradient arena)."""
    pred, loss, grads = train_call(m, VAR, *c, 0)
    return pred.detach().clone(), loss, {k: g.clone() for k, g in grads.items()}


_FRESH = {}


def fresh_run(B, k=0):
    """What a fresh model that made only this training call gives; computed once, never written to."""
    if (B, k) not in _FRESH:
        _FRESH[(B, k)] = run(fresh(), case(B, k))
    return _FRESH[(B, k)]


def same_grads(got, want, label):
    assert set(got) == set(want), (label, sorted(set(got) ^ set(want))[:8])
    bad = [k for k in want if not torch.equal(got[k], want[k])]
    assert not bad, f"{label}: {len(bad)} of {len(want)} gradients differ, e.g. {bad[:5]}"


def same_run(got, want, label):
    assert torch.equal(got[0], want[0]), label + ": prediction"
    assert got[1] == want[1], (label, got[1], want[1])
    same_grads(got[2], want[2], label)


def untouched(m):
    assert all(p.grad is None for p in m.parameters()), "a refused backward assigned a gradient"


# ------------------------------------------------------------------------------------------ training: TrainStep helpers
def step_batches(sizes):
    rs = np.random.RandomState(11)
    out = []
    for i, B in enumerate(sizes):
        inp = synthetic_inputs(B, seed=200 + i, hw=HW, num_classes=CFG["num_classes"])
        inp["t"] = torch.from_numpy(rs.randint(1, 1000, size=(B,))).long()
        inp["eps"] = torch.from_numpy(rs.standard_normal(tuple(inp["x"].shape)).astype(np.float32))
        out.append(inp)
    return out


def step_setup(diff, use_graph):
    m = fill_module_(UNetModel(args=make_args(device=DEV), **CFG), 17).to(DEV).train()
    ema = copy.deepcopy(m).eval().requires_grad_(False)
    opt = FusedAdamW(m.parameters(), lr=1e-4, ema_model=ema, ema_beta=0.9, step_start_ema=3)
    return m, ema, opt, TrainStep(m, diff, opt, seed=3, use_graph=use_graph)


def step_call(step, b):
    loss = step(b["x"].to(DEV), b["context"].to(DEV), b["y"].to(DEV), t=b["t"], noise=b["eps"].to(DEV))
    torch.cuda.synchronize()
    return loss.clone()


def checkpoint(m, ema, opt):
    return ({k: v.clone() for k, v in m.state_dict().items()}, {k: v.clone() for k, v in ema.state_dict().items()},
            opt.state_dict())


def twin_step(diff, use_graph, ckpt, b):
    """A fresh model, EMA copy, optimiser and TrainStep resumed from ``ckpt`` (the state_dict round trip of
    test_fused_adamw_state_dict_round_trip_resumes_bit_exactly) that take the one step ``b`` uninterrupted."""
    m, ema, opt, step = step_setup(diff, use_graph)
    m.load_state_dict(ckpt[0])
    ema.load_state_dict(ckpt[1])
    opt.load_state_dict(ckpt[2])
    return m, ema, opt, step_call(step, b)


def same_state(a, b, label):
    (m_a, ema_a, opt_a, loss_a), (m_b, ema_b, opt_b, loss_b) = a, b
    assert torch.equal(loss_a, loss_b), (label, float(loss_a), float(loss_b))
    for what, x, y in (("parameter", m_a, m_b), ("EMA", ema_a, ema_b)):
        bad = [k for (k, u), v in zip(x.state_dict().items(), y.state_dict().values()) if not torch.equal(u, v)]
        assert not bad, f"{label}: {len(bad)} {what} tensors differ, e.g. {bad[:5]}"
    sa, sb = opt_a.state_dict(), opt_b.state_dict()
    assert sa["wdiff"] == sb["wdiff"] and sorted(sa["state"]) == sorted(sb["state"]) and len(sa["state"]) > 0
    bad = [(i, n) for i, s in sa["state"].items() for n in ("step", "exp_avg", "exp_avg_sq") if not torch.equal(s[n], sb["state"][i][n])]
    assert not bad, f"{label}: AdamW state differs, e.g. {bad[:5]}"


@pytest.fixture
def graph_calls(monkeypatch):
    """Counts the library's graph entry points (the spy of test_default_settings_launch_what_the_parent_launches)."""
    lib, calls = N.lib(), collections.Counter()
    for name in ("wd_graph_begin", "wd_graph_launch", "wd_graph_destroy"):
        def spy(*a, _f=getattr(lib, name), _n=name):
            calls[_n] += 1
            return _f(*a)
        monkeypatch.setattr(lib, name, spy)
    return calls


# ------------------------------------------------------------------------------------------ inference: helpers
def eval_model(cfg=CFG, seed=9, **args_kw):
    return fill_module_(UNetModel(args=make_args(device=DEV, **args_kw), **cfg), seed).to(DEV).eval()


def eval_inputs(B, num_classes=CFG["num_classes"]):
    inp = synthetic_inputs(B, seed=40 + B, hw=HW, num_classes=num_classes)
    return {k: v.to(DEV) for k, v in inp.items()}


def eval_fwd(m, inp, **kw):
    with torch.no_grad():
        out = m(inp["x"], timesteps=inp["t"], context=inp["context"], y=inp["y"], **kw)
    torch.cuda.synchronize()
    return out


def run_plan(eng, P, inp):
    """A plan the caller holds, run the way ``UNetEngine.forward`` runs it."""
    eng.refresh_weights()
    eng.load_inputs(P, inp["x"], inp["t"], inp["context"], inp["y"])
    stream = torch.cuda.current_stream(eng.device).cuda_stream
    P.run_cond(stream)
    P.run_step(stream)
    torch.cuda.synchronize()
    return P.out.clone()


LABELS3 = torch.tensor([1, 7, 10], dtype=torch.int64)


def sample(m, which, seed=3):
    args = make_args(device=DEV)
    diff = Diffusion(noise_steps=T, img_size=IMG, args=args)
    if which == "ddpm":
        out = diff.sampling(m, None, 3, "MOVE", LABELS3, args, seed=seed)
    else:
        out = diff.sampling_ddim(m, None, 3, "MOVE", LABELS3, args, steps=3, seed=seed)
    torch.cuda.synchronize()
    return out.clone()


# ------------------------------------------------------------------------------------------ the premise
def test_fresh_models_agree_bit_for_bit():
    """The premise of every ``torch.equal`` below, one assertion per path: two fresh models give the same bits."""
    for B in (1, 2, 3):
        same_run(run(fresh(), case(B)), fresh_run(B), f"training call, B = {B}")
    inp = eval_inputs(2)
    assert torch.equal(eval_fwd(eval_model(), inp), eval_fwd(eval_model(), inp)), "eval forward"
    for which in ("ddpm", "ddim"):
        assert torch.equal(sample(eval_model(), which), sample(eval_model(), which)), which
    diff = Diffusion(noise_steps=1000, img_size=IMG, args=make_args(device=DEV))
    b = step_batches([2])[0]
    for use_graph in (True, False):
        one, two = step_setup(diff, use_graph), step_setup(diff, use_graph)
        same_state(one[:3] + (step_call(one[3], b),), two[:3] + (step_call(two[3], b),), f"TrainStep(use_graph={use_graph})")
    # captured and eager run the same launches: one twin would do for both
    g, e = step_setup(diff, True), step_setup(diff, False)
    same_state(g[:3] + (step_call(g[3], b),), e[:3] + (step_call(e[3], b),), "TrainStep graph vs eager")


# ------------------------------------------------------------------------------------------ training engine
def test_shapes_that_come_back():
    """B = 2, 3, 2 on one model, nothing released in between: each shape change rebuilds the plan (and drops the scratch of the one
    before), the gradient arena stays.  The third call is the first, both are a fresh model's, and that is the float64 oracle's."""
    m = fresh()
    eng = m.train_engine
    got = []
    for B in (2, 3, 2):
        m.zero_grad(set_to_none=True)
        got.append(run(m, case(B)))
        assert len(eng._tplans) == 1 and eng.holds_plan(eng._live) and eng._live.x_in.shape[0] == B
    same_run(got[2], got[0], "B = 2 after B = 3 against the first B = 2")
    same_run(got[0], fresh_run(2), "B = 2 against fresh")
    same_run(got[1], fresh_run(3), "B = 3 after B = 2 against fresh")
    same_run(got[2], fresh_run(2), "B = 2 after B = 3 against fresh")
    check_against_reference(*got[2], reference64(CFG, VAR, 2, HW, 0, SEEDS), "B = 2 after B = 3")


def test_two_forwards_at_one_shape():
    """``pa = m(xa); pb = m(xb)`` share one cached plan whose saved intermediates are those of xb: the backward of L(pa) is refused -
    no ``param.grad`` assigned (first model) or changed (second model, which holds gradients from an earlier call) -, the backward
    of L(pb) is the fresh single-forward one, and (L(pa) + L(pb)).backward() is refused as well."""
    ca, cb = case(2), case(2, 1)
    m = fresh()
    pa, pb = fwd(m, ca), fwd(m, cb)
    with pytest.raises(RuntimeError, match=STALE):
        loss_of(ca, pa).backward()
    untouched(m)
    lb = loss_of(cb, pb)
    lb.backward()
    want = fresh_run(2, 1)
    assert torch.equal(pb.detach(), want[0]) and float(lb.detach()) == want[1]
    same_grads(grads_of(m), want[2], "L(pb).backward() after the refused L(pa).backward()")
    # a model that already holds gradients: the refused backward leaves the objects and their bits as they were
    held = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    before = {k: g.clone() for k, g in held.items()}
    pa, pb = fwd(m, ca), fwd(m, cb)
    with pytest.raises(RuntimeError, match=STALE):
        loss_of(ca, pa).backward()
    torch.cuda.synchronize()
    now = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    assert set(now) == set(held) and all(now[k] is held[k] for k in held)
    same_grads(now, before, "gradients held across a refused backward")
    # both losses in one backward: the node of pa is refused whichever node runs first
    m2 = fresh()
    pa, pb = fwd(m2, ca), fwd(m2, cb)
    with pytest.raises(RuntimeError, match=STALE):
        (loss_of(ca, pa) + loss_of(cb, pb)).backward()


@pytest.mark.parametrize("B0", [1, 2])
def test_two_forwards_at_two_shapes(B0):
    """The second forward has another batch size, so ``plan_train`` released the first one's plan and scratch.  The first backward
    is refused with the same RuntimeError - at B0 = 2 it used to fail on a copy shape, at B0 = 1 ``copy_`` broadcast d loss / d out
    over three samples and a gradient was assigned.  The second forward's backward is the fresh one."""
    c0, c3 = case(B0), case(3)
    m = fresh()
    p0, p3 = fwd(m, c0), fwd(m, c3)
    with pytest.raises(RuntimeError, match=STALE) as e:
        loss_of(c0, p0).backward()
    assert "released" in str(e.value)
    untouched(m)
    l3 = loss_of(c3, p3)
    l3.backward()
    want = fresh_run(3)
    assert torch.equal(p3.detach(), want[0]) and float(l3.detach()) == want[1]
    same_grads(grads_of(m), want[2], f"B = 3 after an abandoned B = {B0} forward")


def test_second_backward_through_one_forward():
    """``loss.backward(retain_graph=True)`` twice is VALID and leaves exactly twice the single gradient (g + g is exact in fp32).
    Why (``TrainEngine.backward``): the backward list only reads what the forward saved - operand planes, pre-activations,
    GroupNorm statistics, K | V, attention outputs - and every buffer it writes is either its own, with the first writer in list
    order overwriting and later ones adding, or shared scratch refilled before each read.  So the second run repeats the first bit
    for bit and ``backward`` adds it to the ``param.grad`` the first one left, as autograd's accumulation would."""
    c = case(2)
    m = fresh()
    loss = loss_of(c, fwd(m, c))
    loss.backward(retain_graph=True)
    once = grads_of(m)
    same_grads(once, fresh_run(2)[2], "first backward")
    loss.backward(retain_graph=True)
    same_grads(grads_of(m), {k: g + g for k, g in once.items()}, "second backward through the same forward")


def _eval_forward_elsewhere(m):
    m.eval()
    eval_fwd(m, eval_inputs(3))
    m.train()


def _no_grad_forward_same_shape(m):  # (train mode under no_grad is the inference engine too: dropout is 0)
    eval_fwd(m, eval_inputs(2))
    assert m.training


def _sampling(m):
    m.eval()
    sample(m, "ddpm")
    m.train()


def _unrelated_buffers(m):
    if not hasattr(m, "calls_seen"):
        m.register_buffer("calls_seen", torch.zeros(1 << 16, device=DEV))  # no parameter: the engines' weight signature ignores it
    m.calls_seen.add_(1.0)
    torch.full((1 << 20,), float("nan"), device=DEV)  # an allocation that comes and goes


@pytest.mark.parametrize("between", [_eval_forward_elsewhere, _no_grad_forward_same_shape, _sampling, _unrelated_buffers],
                         ids=lambda f: f.__name__.strip("_"))
def test_other_work_between_forward_and_backward(between):
    """What does not go through the training engine leaves a pending backward alone: an eval forward at another batch size, a
    no_grad forward at the same one, a few sampler steps, writes to buffers that are no parameters.  (No parameter changes.)"""
    c = case(2)
    m = fresh()
    pred = fwd(m, c)
    loss = loss_of(c, pred)
    between(m)
    loss.backward()
    want = fresh_run(2)
    assert torch.equal(pred.detach(), want[0]) and float(loss.detach()) == want[1]
    same_grads(grads_of(m), want[2], between.__name__)


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_train_step_sharing_its_model(use_graph, graph_calls):
    """Two steps at B = 2, then ``model(...)`` -> backward under autograd at B = 3 on the same model - ``plan_train`` releases the
    scratch the step's plan and captured graph point into, and the step's own key has not changed -, then a third step at B = 2.
    The step must notice (``TrainEngine.holds_plan``), build and capture again and never launch the old graph; the third step then
    equals, in loss, parameters, EMA and AdamW state, a twin resumed from the checkpoint after step 2 that was never interrupted."""
    diff = Diffusion(noise_steps=1000, img_size=IMG, args=make_args(device=DEV))
    bs = step_batches([2, 2, 2])
    m, ema, opt, step = step_setup(diff, use_graph)
    eng = m.train_engine
    for b in bs[:2]:
        step_call(step, b)
    ckpt = checkpoint(m, ema, opt)
    P_old = step._P
    assert eng.holds_plan(P_old)
    assert dict(graph_calls) == (dict(wd_graph_begin=1, wd_graph_launch=2) if use_graph else {})
    # the interruption: a plain training call at another batch size, its gradients dropped again
    c3 = case(3)
    loss_of(c3, fwd(m, c3)).backward()
    m.zero_grad(set_to_none=True)
    assert not eng.holds_plan(P_old) and step._P is P_old
    graph_calls.clear()
    loss = step_call(step, bs[2])
    assert step._P is not P_old and eng.holds_plan(step._P) and step._P.x_in.shape[0] == 2
    # captured anew, the old graph destroyed and never launched: the one launch is the new graph's
    assert dict(graph_calls) == (dict(wd_graph_begin=1, wd_graph_destroy=1, wd_graph_launch=1) if use_graph else {})
    same_state((m, ema, opt, loss), twin_step(diff, use_graph, ckpt, bs[2]), "third step after the interruption")
    # and a pending autograd backward is refused once the step has run over the plan (same shape: B = 2)
    c2 = case(2)
    pending = loss_of(c2, fwd(m, c2))
    step_call(step, bs[2])
    with pytest.raises(RuntimeError, match=STALE):
        pending.backward()


def test_train_step_on_a_ragged_last_batch():
    """Steps at B = 3, 2, 3 on one TrainStep (accumulate = 1): the third equals a twin resumed from the state after the second."""
    diff = Diffusion(noise_steps=1000, img_size=IMG, args=make_args(device=DEV))
    bs = step_batches([3, 2, 3])
    m, ema, opt, step = step_setup(diff, True)
    for b in bs[:2]:
        step_call(step, b)
    ckpt = checkpoint(m, ema, opt)
    loss = step_call(step, bs[2])
    assert step.optimizer_steps == 3 and step._P.x_in.shape[0] == 3
    same_state((m, ema, opt, loss), twin_step(diff, True, ckpt, bs[2]), "B = 3 after B = 2 after B = 3")


# ------------------------------------------------------------------------------------------ inference engine
_FRESH_EVAL = {}


def fresh_eval(B):
    if B not in _FRESH_EVAL:
        _FRESH_EVAL[B] = eval_fwd(eval_model(), eval_inputs(B))
    return _FRESH_EVAL[B]


def test_cached_plans_come_back():
    m = eval_model()
    eng = m.engine
    seen = {}
    for B in (1, 2, 3, 2, 1):
        assert torch.equal(eval_fwd(m, eval_inputs(B)), fresh_eval(B)), B
        P = eng.plan(B, *HW, L, 0)
        assert P.x_in.shape[0] == B and seen.setdefault(B, P) is P, f"B = {B} was planned twice"
    assert len(eng._plans) == 3


MIX_CFG = dict(CFG, num_classes=339)  # (the interpolation forward draws its writers from the reference's 339)


def _six_keys():
    """(name, batch, keyword arguments of the forward): six distinct plan keys of one interpolation model."""
    return [("B=1", 1, {}), ("B=2", 2, {}), ("B=3", 3, {}), ("maps", 2, dict(return_attention=True)),
            ("writer_keep", 2, dict(writer_keep=torch.tensor([True, False]))), ("mix", 2, dict(mix_rate=0.3))]


def _flat(out):
    return torch.cat([o.reshape(-1) for o in out]) if isinstance(out, tuple) else out


def _mix_fwd(m, B, kw):
    random.seed(5)  # (the pair of writers of a mix_rate forward comes from Python's global generator)
    return _flat(eval_fwd(m, eval_inputs(B, 339), **kw))


_FRESH_MIX = {}


def fresh_mix(name, B, kw):
    if name not in _FRESH_MIX:
        _FRESH_MIX[name] = _mix_fwd(eval_model(MIX_CFG, interpolation=True), B, kw)
    return _FRESH_MIX[name]


@pytest.mark.parametrize("room", [4, 1], ids=["default cache of 4", "WDIFF_PLAN_CACHE=1"])
def test_eviction(room, monkeypatch):
    """Six keys through a cache of ``room`` plans, then the first again: never more than ``room`` plans are held, every output is a
    fresh model's, and the B = 1 plan the test kept from before its eviction still runs and still gives the fresh result (a plan
    owns its buffers; the engine-wide workspace has a fixed size)."""
    assert E.PLAN_CACHE_SIZE == 4, "the default the first case is about"
    monkeypatch.setattr(E, "PLAN_CACHE_SIZE", room)  # (read from WDIFF_PLAN_CACHE at import)
    m = eval_model(MIX_CFG, interpolation=True)
    eng = m.engine
    held = None
    for name, B, kw in _six_keys():
        assert torch.equal(_mix_fwd(m, B, kw), fresh_mix(name, B, kw)), name
        assert 1 <= len(eng._plans) <= room, (name, len(eng._plans))
        if held is None:
            held = next(iter(eng._plans.values()))
            assert held.x_in.shape[0] == 1
    assert all(P is not held for P in eng._plans.values()), "six keys did not evict the first plan"
    first = _six_keys()[0]
    assert torch.equal(run_plan(eng, held, eval_inputs(1, 339)), fresh_mix(*first)), "the evicted plan the test still holds"
    assert torch.equal(_mix_fwd(m, 1, {}), fresh_mix(*first)), "B = 1 planned again after its eviction"
    assert len(eng._plans) <= room and all(P is not held for P in eng._plans.values())


def test_weights_changed_under_cached_plans():
    """One conv weight and one writer row change in place while the plans of B = 1, 2, 3 are cached: each of those same plans then
    gives what a fresh model loaded from the new state_dict gives."""
    m = eval_model()
    eng = m.engine
    plans = {}
    for B in (1, 2, 3):
        eval_fwd(m, eval_inputs(B))
        plans[B] = eng.plan(B, *HW, L, 0)
    row = int(eval_inputs(1)["y"][0])  # the writer of the B = 1 sample
    with torch.no_grad():
        m.input_blocks[1][0].in_layers[2].weight.add_(0.01)
        m.label_emb.weight[row].add_(0.01)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    for B in (1, 2, 3):
        got = eval_fwd(m, eval_inputs(B))
        assert eng.plan(B, *HW, L, 0) is plans[B], "the plan was rebuilt: this case is about cached ones"
        new = eval_model()
        new.load_state_dict(sd)
        assert torch.equal(got, eval_fwd(new, eval_inputs(B))), B
        assert not torch.equal(got, fresh_eval(B)), "the change did not reach the output"


def test_a_sampler_call_between_two_forwards():
    m = eval_model()
    inp = eval_inputs(2)
    first = eval_fwd(m, inp)
    drawn = sample(m, "ddim", seed=7)
    m.eval()  # (the samplers leave the model in train mode, like the reference)
    last = eval_fwd(m, inp)
    assert torch.equal(first, last) and torch.equal(first, fresh_eval(2))
    assert torch.equal(drawn, sample(eval_model(), "ddim", seed=7))
