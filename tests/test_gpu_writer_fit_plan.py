"""The frozen-trunk training plan (``plan_train(rows=...)``): its compact gradient against the full plan's ``label_emb.weight.grad``
(bit for bit) and against float64 autograd of the oracle on the grown table; what its backward list launches; that it leaves the
gradient arena alone, ignores ResBlock dropout, and leaves plans without ``rows`` what they were.

B = 3, y = [r_new, old, r_new], rows = (r_new, r_absent): a row with two samples, a sample whose writer is not fitted, a fitted row
no sample names.  SMALL config (c = ted = 256, 4 x 8 latents); one FULL base case at B = 2 against the full plan only."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet_oracle as U  # noqa: E402
from tests._common import FULL, SMALL  # noqa: E402
from tests._plan_sig import signature  # noqa: E402
from tests._train_ref import DEV, case_inputs, train_call, train_model  # noqa: E402

SEEDS = (31, 77, 5)
HW = (4, 8)
PHOSC_LEN = 20  # > 16 keys: the long-key attention backward writes d(K | V) of the context itself
# launches whose only product is the gradient of a frozen parameter, by function and by ``what``
FROZEN_FNS = {"wd_dw", "wd_dw_group", "wd_transpose_planes", "wd_permute_dw", "wd_colsum_finish_multi"}
FROZEN_WHAT = (":dW", ":T(x", ":dbias", ":dbeta", ":dgamma", ":dkv", "input_blocks.0", "cross.kv", "word_emb.", "time_embed.",
               "time SiLU", "d(context)", "deferred finishes")


def setup(cfg, variant, phosc_len, B, dropout=0):
    """(model with two added rows, x, inp with y = [r_new, old, r_new(, ...)], eps, rows)."""
    m = train_model(dict(cfg, dropout=dropout), variant, phosc_len > 0, SEEDS[0])
    old = cfg["num_classes"]
    r_new, r_absent = m.add_writers(2, init=[4, 7])
    assert (r_new, r_absent) == (old, old + 1)
    x, inp, eps = case_inputs(cfg, B, HW if cfg is SMALL else (8, 16), phosc_len, SEEDS)
    inp["y"] = torch.tensor([r_new, 3, r_new][:B])
    return m, x, inp, eps, (r_new, r_absent)


def run_frozen(m, x, inp, dout, rows, phosc_len):
    """The frozen plan on the same inputs and the same d loss / d pred -> (plan, compact gradient clone)."""
    eng = m.train_engine
    eng.refresh_weights()
    P = eng.plan_train(x.shape[0], x.shape[2], x.shape[3], inp["context"].shape[1], phosc_len, rows=rows)
    eng.load_inputs(P, x.to(DEV), inp["t"].to(DEV), inp["context"].to(DEV), inp["y"].to(DEV),
                    inp["phosc"].to(DEV) if phosc_len else None)
    st = torch.cuda.current_stream(DEV).cuda_stream
    P.run_step(st)
    P.dout.copy_(dout)
    P.run_bwd(st)
    torch.cuda.synchronize()
    return P, P.row_grad.clone()


def full_then_frozen(cfg, variant, phosc_len, B):
    """The full plan through model(...) -> MSELoss -> backward, then what the frozen plan is compared with: the prediction, the
    gradients, and (d loss / d pred as the backward list read it, the full backward list by function and ``what``)."""
    m, x, inp, eps, rows = setup(cfg, variant, phosc_len, B)
    pred, _loss, grads = train_call(m, variant, x, inp, eps, phosc_len)
    eng = m.train_engine
    dout = eng._live.dout.clone()
    full_bwd = [(fn.__name__, what) for fn, _a, what in eng._live.bwd]
    return m, x, inp, eps, rows, pred.detach().clone(), {k: g.clone() for k, g in grads.items()}, (dout, full_bwd)


@functools.lru_cache(maxsize=2)
def reference64(variant, phosc_len):
    """float64 autograd of the oracle on the grown table: d MSE / d label_emb.weight."""
    m, x, inp, eps, rows = setup(SMALL, variant, phosc_len, 3)
    sd = {k: v.detach().cpu().double().requires_grad_(k == "label_emb.weight") for k, v in m.state_dict().items()}
    orc = U.UNetOracle(dict(SMALL, num_classes=m.num_classes), sd, variant, phosc_len > 0)
    pred = orc(x.double(), inp["t"], inp["context"], inp["y"], inp.get("phosc"))
    torch.nn.functional.mse_loss(pred, eps.double()).backward()
    return sd["label_emb.weight"].grad


@pytest.mark.parametrize("variant,phosc_len", [("base", 0), ("phosc", PHOSC_LEN)], ids=["base", "phosc"])
def test_compact_gradient_is_the_full_plans_rows(variant, phosc_len):
    m, x, inp, eps, rows, pred, grads, (dout, full_bwd) = full_then_frozen(SMALL, variant, phosc_len, 3)
    arena = m.train_engine.grad_arena()
    before = arena.clone()
    P, g = run_frozen(m, x, inp, dout, rows, phosc_len)
    assert torch.equal(P.out, pred), "the frozen plan's forward is not the training forward"
    full = grads["label_emb.weight"]
    assert tuple(g.shape) == (2, 256)
    assert torch.equal(g.view(torch.int32), full[list(rows)].view(torch.int32)), "compact gradient != rows of the full gradient"
    assert not bool(g[1].any()) and bool(g[0].any()), "the absent row must be exactly zero, the fitted one not"
    ref = reference64(variant, phosc_len)[list(rows)]
    err, rn = float((g.cpu().double() - ref).norm()), float(ref.norm())
    print(f"{variant}: ||g - ref|| = {err:.3e}, ||ref|| = {rn:.3e}, relative {err / rn:.2e}")
    assert err < 2e-4 * rn + 1e-7
    # the arena belongs to the full plan: a frozen backward writes none of it (and carves nothing new)
    assert m.train_engine.grad_arena().data_ptr() == arena.data_ptr() and m.train_engine.grad_arena().numel() == arena.numel()
    assert torch.equal(m.train_engine.grad_arena().view(torch.int32), before.view(torch.int32))
    # the backward list: a sub-list of the full one, then the two row launches
    bwd = [(fn.__name__, what) for fn, _a, what in P.bwd]
    assert [f for f, _ in bwd[-2:]] == ["wd_row_slots", "wd_embedding_bwd"]
    assert len(bwd) < len(full_bwd)
    # (the PHOSC model's a1 is the spatial self-attention: its d(K | V) are data gradients of the tokens and stay)
    hits = [(f, w) for f, w in bwd if f in FROZEN_FNS or any(s in w for s in FROZEN_WHAT)
            if not (variant == "phosc" and ".a1:bwd:dkv" in w)]
    assert variant != "phosc" or any(".a1:bwd:dkv" in w for _f, w in bwd)
    assert not hits, hits[:8]
    it = iter(full_bwd)
    missing = [op for op in bwd[:-2] if op not in it]  # (each found after the previous: order kept)
    assert not missing, f"launches the full list does not have, or in another order: {missing[:5]}"
    kept = {w for _f, w in bwd}
    assert "emb_layers(all):dX0" in kept and "emb SiLU:bwd" in kept and any(w.endswith(".conv1:dfilm") for w in kept)
    assert not any(w.endswith(":dfilm") for _f, w in full_bwd if (_f, w) not in bwd), "a FiLM sum was dropped"
    assert P.bwd_segments == [] and P.dropouts == []


def test_poisoned_arena_survives_a_frozen_backward():
    m, x, inp, eps, rows, pred, grads, (dout, _) = full_then_frozen(SMALL, "base", 0, 3)
    arena = m.train_engine.grad_arena()
    arena.view(torch.int32).fill_(0x7FBADBAD)
    _P, g = run_frozen(m, x, inp, dout, rows, 0)
    assert bool((m.train_engine.grad_arena().view(torch.int32) == 0x7FBADBAD).all())
    assert bool(torch.isfinite(g).all())
    assert all(p.grad is None or p.grad.data_ptr() != g.data_ptr() for p in m.parameters())


def test_frozen_plan_alone_carves_no_arena():
    m, x, inp, eps, rows = setup(SMALL, "base", 0, 3)
    eng = m.train_engine
    eng.refresh_weights()
    P = eng.plan_train(3, *HW, inp["context"].shape[1], 0, rows=rows)
    assert eng._arena is None and not eng._grad and not eng._carve_order and eng._cut_closures is None
    assert P.row_grad is not None and tuple(P.row_grad.shape) == (2, 256)


def test_dropout_is_not_applied_to_a_frozen_trunk():
    """A model built with dropout=0.1 gives the same compact gradient bits as the same weights with dropout=0."""
    m0, x, inp, eps, rows, pred, _grads, (dout, _) = full_then_frozen(SMALL, "base", 0, 3)
    _P0, g0 = run_frozen(m0, x, inp, dout, rows, 0)
    m1, *_ = setup(SMALL, "base", 0, 3, dropout=0.1)
    assert m1.training and any(mod.p == 0.1 for mod in m1.modules() if isinstance(mod, torch.nn.Dropout))
    P1, g1 = run_frozen(m1, x, inp, dout, rows, 0)
    assert torch.equal(P1.out, pred) and not P1.dropouts
    assert torch.equal(g1.view(torch.int32), g0.view(torch.int32))


def test_full_base_against_the_full_plan():
    m, x, inp, eps, rows, pred, grads, (dout, full_bwd) = full_then_frozen(FULL, "base", 0, 2)
    P, g = run_frozen(m, x, inp, dout, rows, 0)
    assert torch.equal(P.out, pred)
    assert torch.equal(g.view(torch.int32), grads["label_emb.weight"][list(rows)].view(torch.int32))
    assert not bool(g[1].any()) and bool(g[0].any())
    assert len(P.bwd) < len(full_bwd)


def test_plans_without_rows_are_what_they_were():
    m, x, inp, eps, rows = setup(SMALL, "base", 0, 3)
    eng = m.train_engine
    eng.refresh_weights()
    L = inp["context"].shape[1]

    def describe(P):
        return signature(eng, P), [(fn.__name__, what) for fn, _a, what in P.bwd], list(P.bwd_segments)

    key0, _, r0 = eng._train_key(3, *HW, L, 0, None)
    assert r0 is None and key0 == (3, *HW, L, 0, eng.npass), "the cache key of a plan without rows changed"
    before = describe(eng.plan_train(3, *HW, L, 0))
    eng.plan_train(3, *HW, L, 0, rows=rows)
    after = describe(eng.plan_train(3, *HW, L, 0))
    assert before == after
    assert eng._train_key(3, *HW, L, 0, None, rows)[0] != key0
    assert eng._train_key(3, *HW, L, 0, None, rows)[0] != eng._train_key(3, *HW, L, 0, None, rows[::-1])[0]
    for bad, msg in (((rows[0], rows[0]), "distinct"), ((m.num_classes,), "lie in"), ((), "1 .. 64")):
        with pytest.raises(ValueError, match=msg):
            eng.plan_train(3, *HW, L, 0, rows=bad)
    with pytest.raises(ValueError, match="label_drop"):
        eng.plan_train(3, *HW, L, 0, label_drop=0.5, rows=rows)
