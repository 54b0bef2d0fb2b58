"""The HIP forward and the training gradients at the model shapes of tests/_shapes.py: head counts 1 / 2 / 8, two ResBlocks per level,
widths 96 / 128 / 160 / 256, channel multipliers (1, 2) and (1, 2, 4), latent maps 8 x 64, 16 x 32, 8 x 16 and 6 x 26, base and PHOSC.

  golden     the forward against the reference's own output (tests/golden/fwd_shape_<tag>.npz) at test_forward_matches_reference_golden's bars;
  plans      engine.plan at every batch of the sweep (B = 1 .. 130; .. 40 for the 512-token maps): no exception, no GEMM that wd_gemm_check
             refuses, and the batch sizes at which the kernel family changes are exactly ``FAMILY_THRESHOLDS`` - the batch lists of the
             forward test were checked this way: they hold b - 1 and b of every such change (tests/test_shapes_host.py);
  forward    every (tag, B) of ``BATCHES`` against the float64 oracle, each sample on its own, max_rel < 1e-4 (the bar of
             test_full_size_properties_b64 and of tests/test_gpu_batch_thresholds.py), a second call bit-identical;
  forms      the plans take the kernels the tags are there for (a later planner change must not move the tests off them silently);
  gradients  model in train mode -> MSELoss -> backward at B = 3 against float64 autograd of the oracle, tests/_train_ref.py's bars.

One model per tag (weights of seed 7, the golden's), built on first use and kept for the module; the oracle's outputs come from one
pool of distinct samples per tag, computed once in chunks of 32.  ``pytest -s`` prints the worst error of every case;
profiles/shape_sweep_errors.txt is that output."""
import gc
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet_oracle as U  # noqa: E402
from tests._common import golden_state_dict, load_golden, make_args, max_rel  # noqa: E402
from tests._plan_sig import families, release, signature  # noqa: E402
from tests._shapes import BATCHES, CTX_LEN, FAMILY_THRESHOLDS, GRAD_TAGS, SHAPES, phosc_len, sweep_limit  # noqa: E402
from tests._train_ref import case_inputs, check_against_reference, reference64, train_call, train_model  # noqa: E402
from worddiffusion_amd import UNetModel, UNetModelPhosc  # noqa: E402
from worddiffusion_amd.synthetic import fill_module_, synthetic_inputs, synthetic_tensor  # noqa: E402

DEV = "cuda:0"
SEED_W = 7        # the seed of the goldens' weights
SEED_POOL = 11
ORACLE_CHUNK = 32
TAGS = list(SHAPES)
FORWARD_CASES = [(tag, B) for tag in TAGS for B in BATCHES[tag]]
ONE_LAUNCH = ": gn + proj_in + a1 + a2 + ff + proj_out (fused)"   # the ``what`` of the one-launch SpatialTransformer


def pool_inputs(tag, n) -> dict:
    cfg, _, hw = SHAPES[tag]
    inp = synthetic_inputs(n, SEED_POOL, hw=hw, num_classes=cfg["num_classes"], phosc_len=phosc_len(tag))
    # every sample is its own: a kernel that read a neighbour's row, timestep, word or writer would not get away with it
    assert len({inp["x"][b].numpy().tobytes() for b in range(n)}) == n
    for k in ("t", "context", "y"):
        assert len({inp[k][b].numpy().tobytes() for b in range(n)}) > n // 2, k
    return inp


def oracle_pool(tag, inp, count):
    """float64 UNetOracle over the first ``count`` samples of the pool, at most ORACLE_CHUNK at a time."""
    cfg, variant, _ = SHAPES[tag]
    sd = {k: torch.from_numpy(synthetic_tensor(k, s, SEED_W)).double() for k, s in U.state_dict_shapes(cfg, variant)}
    orc = U.UNetOracle(cfg, sd, variant, variant == "phosc")
    assert orc.dtype == torch.float64
    outs = []
    with torch.no_grad():
        for b0 in range(0, count, ORACLE_CHUNK):
            s = slice(b0, min(count, b0 + ORACLE_CHUNK))
            outs.append(orc(inp["x"][s], inp["t"][s], inp["context"][s], inp["y"][s], inp["phosc"][s] if variant == "phosc" else None))
    return torch.cat(outs)


class _Tags:
    """Per tag, made on first use and kept for the module: the model on the device, the pool's inputs and (``ref=True``) the oracle's
    outputs over it."""

    def __init__(self):
        self._t = {}

    def get(self, tag, ref=False):
        if tag not in self._t:
            cfg, variant, _ = SHAPES[tag]
            cls = UNetModel if variant == "base" else UNetModelPhosc
            m = fill_module_(cls(args=make_args(device=DEV, phosc=1 if variant == "phosc" else 0), **cfg), SEED_W).to(DEV).eval()
            self._t[tag] = dict(model=m)
        entry = self._t[tag]
        if ref and "ref" not in entry:
            count = max(BATCHES[tag])
            entry["inp"] = pool_inputs(tag, count)
            t0 = time.time()
            entry["ref"] = oracle_pool(tag, entry["inp"], count)
            print(f"\n[shapes] float64 oracle, {tag}: {count} samples in {time.time() - t0:.1f} s of CPU")
        return entry


@pytest.fixture(scope="module")
def tags():
    t = _Tags()
    yield t
    for v in t._t.values():
        release(v["model"].engine)


def call(m, variant, x, t, ctx, y, phosc):
    if variant == "base":
        return m(x.to(DEV), None, original_images=None, timesteps=t.to(DEV), context=ctx.to(DEV), y=y.to(DEV))
    return m(x.to(DEV), phosc.to(DEV), timesteps=t.to(DEV), context=ctx.to(DEV), y=y.to(DEV))


def plan_signatures(eng, tag, batches) -> dict:
    """{B: signature of the forward's plan at B}; plans only (nothing but ``refresh_weights`` and buffer fills launch)."""
    _, _, (h, w) = SHAPES[tag]
    eng.refresh_weights()
    out = {}
    try:
        for i, B in enumerate(batches):
            out[B] = signature(eng, eng.plan(B, h, w, CTX_LEN, phosc_len(tag)))
            eng._plans.clear()
            eng._cur_plan = None
            if i % 16 == 15:
                gc.collect()
    finally:
        release(eng)
    return out


# ------------------------------------------------------------------------------------------ a. the reference's own output
@pytest.mark.parametrize("tag", TAGS)
def test_forward_matches_the_reference_golden(tags, golden_dir, tag):
    _, variant, hw = SHAPES[tag]
    g = load_golden(golden_dir, "fwd_shape_" + tag)
    assert int(g["seed"]) == SEED_W
    m = tags.get(tag)["model"]
    sd = golden_state_dict(g)
    for k, v in m.state_dict().items():   # (the module's model IS the golden's: same keys, same values)
        assert torch.equal(v.cpu(), sd[k]), k
    phosc = torch.from_numpy(g["phosc"]) if variant == "phosc" else None
    try:
        with torch.no_grad():
            out = call(m, variant, *(torch.from_numpy(g[k]) for k in ("x", "t", "context", "y")), phosc).cpu()
    finally:
        release(m.engine)
    assert out.shape == tuple(g["out"].shape) == (2, 4) + hw and out.dtype == torch.float32
    err = max_rel(out, g["out"])
    print(f"\n[shapes] {tag} golden: max_rel {err:.3e} against the reference")
    assert err < 1e-3, (tag, err)
    assert err < 1e-4, (tag, err)


# ------------------------------------------------------------------------------------------ b. plans build everywhere
@pytest.mark.parametrize("tag", TAGS)
def test_plans_build_at_every_batch(tags, tag):
    """Every batch of the sweep plans (an exception fails the test at its B), no GEMM is one wd_gemm_check refuses, and the kernel
    family changes at the batch sizes tests/_shapes.FAMILY_THRESHOLDS lists and nowhere else."""
    eng = tags.get(tag)["model"].engine
    limit = sweep_limit(tag)
    sigs = plan_signatures(eng, tag, range(1, limit + 1))
    for B, sig in sigs.items():
        refused = [what for _, _, what, form in sig if form.startswith("REFUSED")]
        assert not refused, (tag, B, refused[:4])
    changes = []
    for b in range(2, limit + 1):
        lo, hi = families(sigs[b - 1]), families(sigs[b])
        if lo != hi:
            changes.append(b)
            gone = {k: n - hi.get(k, 0) for k, n in lo.items() if n > hi.get(k, 0)}
            new = {k: n - lo.get(k, 0) for k, n in hi.items() if n > lo.get(k, 0)}
            print(f"\n[shapes] {tag} B = {b}: - {gone} + {new}")
    plain = [b for b in range(2, limit + 1) if sigs[b] != sigs[b - 1]]
    print(f"\n[shapes] {tag}: the signature changes at B = {plain}; the kernel family at B = {changes}")
    assert tuple(changes) == FAMILY_THRESHOLDS[tag], "update FAMILY_THRESHOLDS (the batch lists follow from it)"


# ------------------------------------------------------------------------------------------ c. the float64 oracle
@pytest.mark.parametrize("tag,B", FORWARD_CASES, ids=[f"{t}-{B}" for t, B in FORWARD_CASES])
def test_forward_matches_the_oracle(tags, tag, B):
    _, variant, hw = SHAPES[tag]
    entry = tags.get(tag, ref=True)
    m, inp = entry["model"], entry["inp"]
    args = [inp[k][:B] for k in ("x", "t", "context", "y")] + [inp["phosc"][:B] if variant == "phosc" else None]
    try:
        with torch.no_grad():
            out = call(m, variant, *args)
            assert torch.equal(call(m, variant, *args), out), "a second call returned other bits"
        out = out.cpu()
    finally:
        release(m.engine)
    assert out.shape == (B, 4) + hw and out.dtype == torch.float32
    assert torch.isfinite(out).all()
    errs = [max_rel(out[b], entry["ref"][b]) for b in range(B)]
    worst = max(range(B), key=errs.__getitem__)
    print(f"\n[shapes] {tag} B = {B}: worst sample {worst}, max_rel {errs[worst]:.3e} against the oracle")
    assert errs[worst] < 1e-4, [(b, e) for b, e in enumerate(errs) if e >= 1e-4]


# ------------------------------------------------------------------------------------------ d. the forms the tags are there for
def _ops(sig, fn=None, what=None):
    return [(name, w, form) for _, name, w, form in sig if (fn is None or name == fn) and (what is None or what in w)]


@pytest.mark.parametrize("tag", ["heads1", "heads2"])
def test_few_heads_take_the_folded_forms_of_the_320_channel_blocks(tags, tag):
    """d = 320 / 160.  The three 8 x 32 blocks: below 192 panels the folded pair writing planes for the two-source tail (B = 47); from
    192 panels the pair and wd_ff_fused with proj_out (B = 48, 63); once proj_in's GroupNorm staging fills the chip as well the
    one-launch form (B = 64).  The folds of all four blocks run in the conditioning phase throughout."""
    sig = plan_signatures(tags.get(tag)["model"].engine, tag, (47, 48, 63, 64))
    for B in (47, 48, 63, 64):
        assert len(_ops(sig[B], "wd_xattn_fold")) == 8, B   # a1 and a2 of in1.1, mid.1, out2.1, out3.1
        assert not _ops(sig[B], "wd_attention", ".tb0."), B
    assert len(_ops(sig[47], "wd_xattn_planes", "a1+a2:folded + planes")) == 4 and not _ops(sig[47], "wd_ff_fused")
    for B in (48, 63):
        assert len(_ops(sig[B], "wd_xattn_pair", "a1+a2:folded")) == 3, B
        ff = _ops(sig[B], "wd_ff_fused")
        assert len(ff) == 3 and all(w.endswith(".ff + proj_out (fused)") and form.startswith("no front, proj_out folded") for _, w, form in ff), ff
    one = _ops(sig[64], "wd_ff_fused")
    assert len(one) == 3 and all(w.endswith(ONE_LAUNCH) and form.startswith("front, proj_out folded") for _, w, form in one), one
    assert not _ops(sig[64], "wd_xattn_pair") and len(_ops(sig[64], "wd_xattn_planes")) == 1   # (the 4 x 16 block keeps the chain)


def test_eight_heads_run_plain_attention_in_front_of_the_fused_tail(tags):
    """heads * L = 80: wd_xattn_supported refuses the fold, both cross-attentions of every block are wd_attention launches
    (nk = 10, d = 40), and the 8 x 32 blocks still end in wd_ff_fused at B = 48."""
    sig = plan_signatures(tags.get("heads8")["model"].engine, "heads8", (47, 48))
    for B in (47, 48):
        assert not [n for _, n, _, _ in sig[B] if n.startswith("wd_xattn")], B
        att = [w for _, w, _ in _ops(sig[B], "wd_attention", ".tb0.")]
        assert sorted(att) == sorted(f"{blk}.tb0.{a}" for blk in ("in1.1", "mid.1", "out2.1", "out3.1") for a in ("a1", "a2")), att
    assert not _ops(sig[47], "wd_ff_fused")
    ff = _ops(sig[48], "wd_ff_fused")
    assert len(ff) == 3 and all(w.endswith(".ff + proj_out (fused)") and form.startswith("no front") for _, w, form in ff), ff


def test_a_256_channel_model_takes_no_320_channel_form(tags):
    sigs = plan_signatures(tags.get("emb256")["model"].engine, "emb256", BATCHES["emb256"])
    for B, sig in sigs.items():
        names = {n for _, n, _, _ in sig}
        assert "wd_ff_fused" not in names and not [n for n in names if n.startswith("wd_xattn")], (B, sorted(names))
        assert len(_ops(sig, "wd_attention", ".tb0.")) == 8, B


def test_a_ragged_map_never_takes_the_one_launch_form(tags):
    """hw = 156: a 64-token panel would straddle two samples.  wd_ff_fused itself is taken from 192 panels (B = 79), without a front."""
    sigs = plan_signatures(tags.get("full_6x26")["model"].engine, "full_6x26", range(1, sweep_limit("full_6x26") + 1))
    for B, sig in sigs.items():
        ff = _ops(sig, "wd_ff_fused")
        assert all(form.startswith("no front") and not w.endswith(ONE_LAUNCH) for _, w, form in ff), (B, ff)
        assert bool(ff) == (B >= 79), B


def test_the_phase_upsample_is_planned_only_where_its_consumer_reads_it(tags):
    """mult12: the decoder GroupNorm behind the Upsample has 640 + 320 channels in groups of 30, which straddle the concat - the
    Upsample stays on the 9-tap form although its 64 x 320 tiles would fill the chip from B = 32, and the norm materialises the
    concat.  heads2 (320 + 320, groups of 20): the four-phase form from B = 64, read by the two-source GroupNorm launch."""
    sig = plan_signatures(tags.get("mult12")["model"].engine, "mult12", (31, 32, 33, 64, 128))
    for B, s in sig.items():
        assert not _ops(s, what="(4 phases)") and len(_ops(s, "wd_gemm", "out1.2.conv")) == 1, B
        assert len(_ops(s, "wd_copy2d", "out2.0.gn1:concat")) == 2, B
    sig = plan_signatures(tags.get("heads2")["model"].engine, "heads2", (63, 64))
    assert not _ops(sig[63], what="(4 phases)")
    assert len(_ops(sig[64], "wd_gemm", "out1.1.conv (4 phases)")) == 1 and _ops(sig[64], "wd_gn_apply2", "out2.0.gn1:apply")


# ------------------------------------------------------------------------------------------ e. gradients
@pytest.mark.parametrize("tag", GRAD_TAGS)
def test_training_gradients(tag):
    cfg, variant, hw = SHAPES[tag]
    B, plen = 3, phosc_len(tag)
    seeds = (55, 103, 3)
    x, inp, eps = case_inputs(cfg, B, hw, plen, seeds)
    m = train_model(cfg, variant, plen > 0, seeds[0])
    pred, loss, grads = train_call(m, variant, x, inp, eps, plen)
    check_against_reference(pred, loss, grads, reference64(cfg, variant, B, hw, plen, seeds), f"[shapes] {tag} gradients B={B} {hw}")
