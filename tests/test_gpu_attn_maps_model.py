"""forward(return_attention=): the per-character attention maps of the three tapped SpatialTransformers against the reference's
own (tests/golden/attn_maps_full.npz, FULL: the only geometry the reference's maps path runs at) and, at the geometries it cannot
run, against the oracle's attn2 softmax (tests/_xmap_ref.py record_maps).  Bars: 1e-4 max-norm relative, the split-bf16 bar of
tests/test_gpu_model.py for a forward, on eps and maps alike; 2e-5 between the chained and the one-launch SpatialTransformer
(tests/test_gpu_st_fused.py)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet_oracle as U  # noqa: E402
from tests import _xmap_ref as X  # noqa: E402
from tests._common import DEEP, FULL, SMALL, load_golden, make_args, max_rel  # noqa: E402
from worddiffusion_amd import UNetModel, UNetModelPhosc  # noqa: E402
from worddiffusion_amd.synthetic import fill_module_, synthetic_inputs, synthetic_tensor  # noqa: E402

DEV = "cuda:0"
TOL = 1e-4


def _model(cfg, seed, cls=UNetModel, **kw):
    return fill_module_(cls(args=make_args(device=DEV, **kw), **cfg), seed).to(DEV).eval()


def _call(m, inp, **kw):
    with torch.no_grad():
        return m(inp["x"].to(DEV), None, original_images=None, timesteps=inp["t"].to(DEV), context=inp["context"].to(DEV),
                 y=inp["y"].to(DEV), **kw)


def _oracle(cfg, seed):
    sd = {k: torch.from_numpy(synthetic_tensor(k, s, seed)) for k, s in U.state_dict_shapes(cfg, "base")}
    return U.UNetOracle(cfg, sd, "base", False)


def _launches(P):
    return [(fn.__name__, what) for fn, _, what in P.step]


def test_full_matches_the_reference_maps(golden_dir):
    g = load_golden(golden_dir, "attn_maps_full")
    m = _model(FULL, int(g["seed"]))
    inp = {k: torch.from_numpy(g[k]) for k in ("x", "t", "context", "y")}
    plain = _call(m, inp)
    out = _call(m, inp, return_attention=True)
    assert len(out) == 4 and all(o.dtype == torch.float32 for o in out)
    eps, maps = out[0], out[1:]
    assert torch.equal(eps, plain)  # B = 2 is below the one-launch SpatialTransformer's threshold: the same launches
    e = max_rel(eps.cpu(), g["eps"])
    print(f"ERR forward eps vs reference: {e:.2e}")
    assert e < TOL
    for name, mp in zip(("attn1", "attn2", "attn3"), maps):
        assert tuple(mp.shape) == tuple(g[name].shape), name
        e = max_rel(mp.cpu(), g[name])
        print(f"ERR forward {name} vs reference: {e:.2e}")
        assert e < TOL, name
        assert float((mp.double().sum(-1) - FULL["num_heads"]).abs().max()) < 1e-5
    # the reference's own tuple: maps replicated to 64 x 256, and the word encoder's output
    ref = _call(m, inp, return_attention="reference")
    assert len(ref) == 5 and torch.equal(ref[0], plain)
    for big, mp, f in zip(ref[1:4], maps, (8, 16, 8)):
        assert tuple(big.shape) == (2, 64, 256, 10)
        assert torch.equal(big, mp.repeat_interleave(f, 1).repeat_interleave(f, 2))
    assert tuple(ref[4].shape) == (2, 10, 320) and ref[4].dtype == torch.float32
    e = max_rel(ref[4].cpu(), g["context_out"])
    print(f"ERR forward context vs reference: {e:.2e}")
    assert e < TOL
    with pytest.raises(ValueError):
        _call(m, inp, return_attention="maps")


@pytest.mark.parametrize("name,cfg,hw,shapes", [("small", SMALL, (4, 8), [(4, 8), (2, 4), (4, 8)]),
                                                ("deep", DEEP, (4, 8), [(2, 4), (1, 2), (2, 4)])])
def test_other_geometries_match_the_oracle_recorder(monkeypatch, name, cfg, hw, shapes):
    """SMALL and DEEP, B = 3.  DEEP has two ResBlocks per level and attention at one level only: its last input SpatialTransformer
    is input_blocks.5.1, not the first one met."""
    seed, B = 31, 3
    m = _model(cfg, seed)
    inp = synthetic_inputs(B, seed=seed + 2, hw=hw, num_classes=cfg["num_classes"])
    ref_eps, ref = X.record_maps(monkeypatch, _oracle(cfg, seed), inp["x"], inp["t"], inp["context"], inp["y"])
    plain = _call(m, inp)
    eps, *maps = _call(m, inp, return_attention=True)
    assert torch.equal(eps, plain) and max_rel(eps.cpu(), ref_eps) < TOL
    assert m.engine.plan(B, hw[0], hw[1], 10, 0, attn_maps=True).map_taps == \
        (("in1.1", "mid.1", "out3.1") if name == "small" else ("in5.1", "mid.1", "out5.1"))
    for i, (mp, r, s) in enumerate(zip(maps, ref, shapes)):
        assert tuple(mp.shape) == (B, *s, 10) == tuple(r.shape)
        e = max_rel(mp.cpu(), r)
        print(f"ERR forward {name} map {i} vs oracle: {e:.2e}")
        assert e < TOL
        assert float((mp.double().sum(-1) - cfg["num_heads"]).abs().max()) < 1e-5


def test_full_batch_64_leaves_the_default_plan_alone(monkeypatch):
    """The one-launch SpatialTransformer regime: the maps plan runs the three tapped blocks as the chain, the default plan is not
    touched by it."""
    seed, B = 5, 64
    m = _model(FULL, seed)
    inp = synthetic_inputs(B, seed=seed + 2, hw=(8, 32), num_classes=FULL["num_classes"])
    eng = m.engine
    plain = _call(m, inp)
    Pd = eng.plan(B, 8, 32, 10, 0)
    before = _launches(Pd)
    assert any("wd_ff_fused" == fn for fn, _ in before) and not any(fn == "wd_xattn_maps" for fn, _ in before)
    eps, *maps = _call(m, inp, return_attention=True)
    Pm = eng.plan(B, 8, 32, 10, 0, attn_maps=True)
    assert Pm is not Pd and eng.plan(B, 8, 32, 10, 0) is Pd
    assert _launches(Pd) == before and torch.equal(_call(m, inp), plain)
    assert sum(fn == "wd_xattn_maps" for fn, _ in _launches(Pm)) == 3
    # every other launch: the default plan's outside the three tapped blocks, what WDIFF_FUSE_ST=0 plans inside them
    assert Pm.map_taps == ("in1.1", "mid.1", "out3.1")
    tapped = lambda l: l[1].startswith(tuple(t + "." for t in Pm.map_taps))  # noqa: E731
    got = [l for l in _launches(Pm) if l[0] != "wd_xattn_maps"]
    monkeypatch.setattr(eng, "fuse_st", False)
    eng._plans.clear()
    chain = _launches(eng.plan(B, 8, 32, 10, 0))
    assert [l for l in got if not tapped(l)] == [l for l in before if not tapped(l)]
    assert [l for l in got if tapped(l)] == [l for l in chain if tapped(l)]
    assert any(fn == "wd_ff_fused" and what.startswith("out2.1.") for fn, what in got)  # the untapped block keeps its one launch
    e = max_rel(eps.cpu(), plain.cpu())
    print(f"ERR eps of the maps plan vs the default plan, B = 64: {e:.2e}")
    assert e < 2e-5
    sl = slice(30, 34)
    _, ref = X.record_maps(monkeypatch, _oracle(FULL, seed), inp["x"][sl], inp["t"][sl], inp["context"][sl], inp["y"][sl])
    for i, (mp, r) in enumerate(zip(maps, ref)):
        e = max_rel(mp[sl].cpu(), r)
        print(f"ERR forward FULL B = 64 map {i} vs oracle (4 samples): {e:.2e}")
        assert e < TOL


def test_phosc_and_autograd_are_refused_before_any_launch():
    inp = synthetic_inputs(2, seed=3, hw=(4, 8), num_classes=SMALL["num_classes"], phosc_len=12)
    mp = _model(SMALL, 2, UNetModelPhosc, phosc=1)
    with torch.no_grad(), pytest.raises(NotImplementedError):
        mp(inp["x"].to(DEV), inp["phosc"].to(DEV), timesteps=inp["t"].to(DEV), context=inp["context"].to(DEV), y=inp["y"].to(DEV),
           return_attention=True)
    with pytest.raises(NotImplementedError):
        mp.engine.plan(2, 4, 8, 10, 12, attn_maps=True)
    assert not mp.engine._plans
    m = _model(SMALL, 2).train()
    with pytest.raises(NotImplementedError):
        m(inp["x"].to(DEV), None, timesteps=inp["t"].to(DEV), context=inp["context"].to(DEV), y=inp["y"].to(DEV),
          return_attention=True)
    assert m._engine is None or not m.engine._plans
    assert m._train_engine is None


def test_separate_attention_launches_give_the_pair_form_maps_bit_for_bit():
    """WDIFF_FUSE_XATTN_PAIR=0 plans attn1 and attn2 as two launches and the maps launch reads attn2's own input (tok1, NULL, a2);
    the default plans one launch for both and the maps launch runs attn1 again (tok, a1, a2).  tok1 is what the pair kernel holds
    in registers between its two attentions, so the two forms must report the same bits - the maps launch's first attention is
    the step's.  Without the folded cross-attention there is nothing to tap."""
    seed, B = 13, 3
    inp = synthetic_inputs(B, seed=seed + 2, hw=(4, 8), num_classes=SMALL["num_classes"])
    outs = []
    for pair in (True, False):
        m = _model(SMALL, seed)
        m.engine.fuse_xattn_pair = pair
        outs.append(_call(m, inp, return_attention=True))
        names = [fn for fn, _ in _launches(m.engine.plan(B, 4, 8, 10, 0, attn_maps=True))]
        # four SpatialTransformers: one attention launch each, or two
        assert names.count("wd_xattn_maps") == 3
        assert sum(n in ("wd_xattn_pair", "wd_xattn_planes", "wd_xattn_fused") for n in names) == (4 if pair else 8)
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    m = _model(SMALL, seed)
    m.engine.fuse_xattn = False
    with pytest.raises(NotImplementedError):
        _call(m, inp, return_attention=True)
    assert not m.engine._plans
