"""Host side of the model-shape tests (tests/_shapes.py): the float64 / fp32 oracle is pinned to the reference's own forward at every
tag (tests/golden/fwd_shape_<tag>.npz, written by oracle/make_golden_shapes.py), ``worddiffusion_amd``'s classes build the same
state_dict, and the table keeps the properties tests/test_gpu_shapes.py relies on."""
import pytest
import torch

from oracle import unet_oracle as U
from tests._common import golden_state_dict, load_golden, make_args, max_rel
from tests._shapes import BATCHES, CTX_LEN, FAMILY_THRESHOLDS, GRAD_TAGS, PHOSC_LEN, SHAPES, levels, phosc_len, sweep_limit
from worddiffusion_amd import UNetModel, UNetModelPhosc
from worddiffusion_amd.engine import wdirect_fills_chip

TAGS = sorted(SHAPES)


def test_the_table_is_the_sixteen_shapes():
    assert len(SHAPES) == 16 and set(GRAD_TAGS) <= set(SHAPES) and len(GRAD_TAGS) == 11
    for tag, (cfg, variant, hw) in SHAPES.items():
        assert variant in ("base", "phosc") and (variant == "phosc") == tag.startswith("phosc_"), tag
        assert list(BATCHES[tag]) == sorted(set(BATCHES[tag])) and BATCHES[tag][0] == 1, tag
        assert max(BATCHES[tag]) <= 129, tag


@pytest.mark.parametrize("tag", TAGS)
def test_state_dict_layouts_agree(golden_dir, tag):
    """The reference's key / shape list (the golden's) == the oracle's == that of the package's model built on the CPU."""
    cfg, variant, _ = SHAPES[tag]
    g = load_golden(golden_dir, "fwd_shape_" + tag)
    want = [(str(k), str(s)) for k, s in zip(g["keys"], g["shapes"])]
    assert [(k, ",".join(map(str, s))) for k, s in U.state_dict_shapes(cfg, variant)] == want
    cls = UNetModel if variant == "base" else UNetModelPhosc
    m = cls(args=make_args(phosc=1 if variant == "phosc" else 0), **cfg)
    assert [(k, ",".join(map(str, v.shape))) for k, v in m.state_dict().items()] == want


@pytest.mark.parametrize("tag", TAGS)
def test_oracle_matches_the_reference(golden_dir, tag):
    """The fp32 oracle against the reference's output at test_oracle_golden.py's bar; the float64 oracle (the reference of the GPU
    tests) is held to the same bar - it differs from the reference's fp32 arithmetic by that arithmetic's rounding only."""
    cfg, variant, hw = SHAPES[tag]
    g = load_golden(golden_dir, "fwd_shape_" + tag)
    assert int(g["seed"]) == 7 and g["x"].shape == (2, 4) + hw and g["out"].shape == g["x"].shape
    assert ("phosc" in g.files) == (variant == "phosc")
    sd = golden_state_dict(g)
    args = [torch.from_numpy(g[k]) for k in ("x", "t", "context", "y")]
    args.append(torch.from_numpy(g["phosc"]) if variant == "phosc" else None)
    for dtype in (torch.float32, torch.float64):
        orc = U.UNetOracle(cfg, {k: v.to(dtype) for k, v in sd.items()}, variant, variant == "phosc")
        assert orc.dtype == dtype
        with torch.no_grad():
            out = orc(*args)
        err = max_rel(out, g["out"])
        print(f"\n[shapes] {tag} {str(dtype)[6:]} oracle against the reference: max_rel {err:.2e}")
        assert err < 2e-5, (tag, dtype, err)


@pytest.mark.parametrize("tag", TAGS)
def test_shape_is_a_valid_reference_model(tag):
    """Base tags: the context is as wide as every level that has a SpatialTransformer (attn1 is built without context_dim and called
    with the context).  Every level's map halves evenly into the next."""
    cfg, variant, _ = SHAPES[tag]
    lv = levels(tag)
    if variant == "base":
        for ch, _, st in lv:
            assert not st or cfg["context_dim"] == ch, (tag, ch)
        assert cfg["context_dim"] == lv[-1][0], "the middle block's SpatialTransformer runs at the lowest level's width"
    for (_, (h, w), _), (_, (h2, w2), _) in zip(lv, lv[1:]):
        assert h % 2 == 0 and w % 2 == 0 and (h2, w2) == (h // 2, w // 2), tag
    assert all(ch % 32 == 0 for ch, _, _ in lv), "GroupNorm32"
    assert all(ch % cfg["num_heads"] == 0 for ch, _, st in lv), tag


def _first(pred, limit):
    return next((b for b in range(1, limit + 1) if pred(b)), None)


def hand_thresholds(tag) -> dict:
    """The planner rules that can be derived by hand, inside the sweep's range: {first batch at which the rule holds: why}.
      * 192 panels: wd_ff_fused (and with it the one-launch SpatialTransformer) is taken once a 320-channel level with a
        SpatialTransformer has (B hw + 63) // 64 >= 192 panels of 64 tokens (engine._ff_fills_chip; wd_ff_supported: c == 320);
      * the four-phase Upsample: wdirect_fills_chip(B * 4 * hw, cout) over the map the Upsample reads (engine._resample)."""
    out = {}
    lv = levels(tag)
    limit = sweep_limit(tag)
    for ch, (h, w), st in lv:
        if st and ch == 320:
            b = _first(lambda b: (b * h * w + 63) // 64 >= 192, limit)
            if b:
                out[b] = f"192 panels at {h} x {w}"
    for ch, (h, w), _ in lv[1:]:  # (the Upsample behind level i's last decoder block keeps its width)
        b = _first(lambda b: wdirect_fills_chip(b * 4 * h * w, ch), limit)
        if b:
            out.setdefault(b, f"phase Upsample from {h} x {w}, {ch} channels")
    return out


def test_hand_thresholds_are_the_ones_the_issue_names():
    assert set(hand_thresholds("heads2")) == {48, 64}
    assert set(hand_thresholds("mult12")) == {32}            # (its SpatialTransformers are 640 wide: no wd_ff_fused)
    assert set(hand_thresholds("full_8x64")) == {24, 32} and set(hand_thresholds("full_16x32")) == {24, 32}
    assert set(hand_thresholds("full_8x16")) == {96, 128}
    assert 79 in hand_thresholds("full_6x26")
    assert hand_thresholds("emb160") == {} and hand_thresholds("mult124") == {} and hand_thresholds("phosc_emb128") == {}
    assert set(hand_thresholds("phosc_heads8")) == {48, 64}


@pytest.mark.parametrize("tag", TAGS)
def test_batch_lists_straddle_the_hand_thresholds(tag):
    assert max(BATCHES[tag]) <= sweep_limit(tag)
    for b, why in hand_thresholds(tag).items():
        assert b - 1 in BATCHES[tag] and b in BATCHES[tag], (tag, b, why)
    for b in FAMILY_THRESHOLDS[tag]:
        assert 2 <= b <= sweep_limit(tag) and b - 1 in BATCHES[tag] and b in BATCHES[tag], (tag, b)
    assert any(b % 2 for b in BATCHES[tag][1:]), "a ragged tail"
    assert phosc_len(tag) in (0, PHOSC_LEN) and CTX_LEN == SHAPES[tag][0]["max_seq_len"]
