"""Training dropout (ResBlock ``dropout > 0``) on the HIP path, held to the host mask of tests/_dropout_ref.py:

  1. ``wd_gn_apply_dropout``: the planes are bit-zero exactly where the host mask drops, the kept values are the plain kernel's times
     float32(1 / (1 - p)) within that kernel's own bound, raw planes and the columns outside the norm are untouched, and a launch on a
     shard of the batch reproduces the rows of the whole-batch launch bit for bit;
  2. ``wd_gn_bwd_{stats,apply,fused}_dropout`` on dz == the existing entry points on the host-premasked dz, bit for bit (the parent's
     kernels are the yardstick);
  3. ``model(...) -> MSELoss -> backward()`` of a ``dropout=0.1`` model against the float64 oracle with the host mask patched into its
     ResBlock;
  4. ``TrainStep``: a replayed graph draws a new mask (device-read row base), the second step meets the oracle at its own rows, a fresh
     TrainStep with the same seed reproduces the first step;
  5. eval mode, train mode without autograd, and the plan of a ``dropout=0`` model."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import ddpm_oracle as D  # noqa: E402
from oracle import unet_oracle as U  # noqa: E402
from tests import _dropout_ref as R  # noqa: E402
from tests._common import FULL, make_args, max_rel  # noqa: E402
from worddiffusion_amd import Diffusion, UNetModel, UNetModelPhosc  # noqa: E402
from worddiffusion_amd import _native as N  # noqa: E402
from worddiffusion_amd import dropout as DO  # noqa: E402
from worddiffusion_amd.synthetic import fill_module_, synthetic_inputs, synthetic_tensor  # noqa: E402

DEV = "cuda:0"
SEED, LAYER = 1234, 5
ROW_BASE, ROW_BASE_DEV = 5, 2  # the struct's row base and the device word added to it: sample b is global row 7 + b


def _st():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def unplanes(p):
    return p[0].float() + p[1].float()


def drop_args(p, row_base=ROW_BASE, row_dev=None, seed=SEED, layer=LAYER):
    d = DO.WdDropout()
    d.seed, d.row_base, d.row_base_dev = seed, row_base, None if row_dev is None else row_dev.data_ptr()
    d.tag, d.thr, d.scale = R.tag(layer), R.threshold(p), float(R.scale(p))
    return d


def gn_stats(lib, xd, B, hw, c):
    nck = lib.wd_gn_nchunk(hw)
    part = torch.zeros(B, nck, 32, 2, dtype=torch.float64, device=DEV)
    N.check(lib.wd_gn_stats(xd.data_ptr(), c, B, hw, c, c // 32, part.data_ptr(), _st()), "stats")
    return part, nck


# ------------------------------------------------------------------------------------------ 1. forward kernel
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("B,hw,c,silu,c_off,ctot", [(2, 32, 64, 1, 0, 64), (1, 100, 64, 0, 0, 64), (3, 128, 320, 1, 320, 640)])
def test_gn_apply_dropout(B, hw, c, silu, c_off, ctot, p):
    lib = N.lib()
    g = torch.Generator().manual_seed(hw + c)
    x = torch.randn(B * hw, c, generator=g) * 2 + 0.5
    gamma, beta = torch.randn(ctot, generator=g), torch.randn(ctot, generator=g)
    ref = F.group_norm(x.double().reshape(B, hw, c).permute(0, 2, 1), 32, gamma[c_off:c_off + c].double(),
                       beta[c_off:c_off + c].double(), 1e-5)
    if silu:
        ref = F.silu(ref)
    ref = ref.permute(0, 2, 1).reshape(B * hw, c)
    keep = torch.from_numpy(R.keep_mask(SEED, ROW_BASE + ROW_BASE_DEV, B, hw, c, LAYER, p)).reshape(B * hw, c)
    want = ref * keep.double() * float(R.scale(p))
    want_raw = c_off != 0
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    part, nck = gn_stats(lib, xd, B, hw, c)
    row_dev = torch.tensor([ROW_BASE_DEV], dtype=torch.int64, device=DEV)
    d = drop_args(p, row_dev=row_dev)

    def launch(x_t, part_t, b, dd):
        pl = torch.full((2, b * hw, ctot), float("nan"), dtype=torch.bfloat16, device=DEV)
        raw = torch.full_like(pl, float("nan")) if want_raw else None
        N.check(lib.wd_gn_apply_dropout(x_t.data_ptr(), c, b, hw, c, c // 32, part_t.data_ptr(), nck, c // 32, gd.data_ptr(),
                                        bd.data_ptr(), 1e-5, silu, pl[0].data_ptr(), pl[1].data_ptr(), ctot, c_off,
                                        raw[0].data_ptr() if want_raw else None, raw[1].data_ptr() if want_raw else None,
                                        C.byref(dd), _st()), "apply+dropout")
        torch.cuda.synchronize()
        return pl.cpu(), None if raw is None else raw.cpu()

    pl, raw = launch(xd, part, B, d)
    mine = pl[:, :, c_off:c_off + c]
    bits = mine.contiguous().view(torch.int16)
    assert not bool(bits[:, ~keep].any()), "a dropped element is not bit-zero in both planes"
    got = unplanes(mine)
    err = max_rel(got, want)
    print(f"max_rel {err:.2e}, kept share {float(keep.float().mean()):.4f}")
    assert err < 3e-5
    big = ref.abs() > 1e-3
    assert torch.equal((got != 0)[big], keep[big])
    if want_raw:
        assert max_rel(unplanes(raw[:, :, c_off:c_off + c]), x) < 1e-5
        assert bool(torch.isnan(raw[:, :, :c_off].float()).all()) and bool(torch.isnan(raw[:, :, c_off + c:].float()).all())
    assert bool(torch.isnan(pl[:, :, :c_off].float()).all()) and bool(torch.isnan(pl[:, :, c_off + c:].float()).all())
    if B > 1:  # a shard: samples 1.. of the batch, keyed with row_base + 1
        pl1, _ = launch(xd[hw:], part[1:], B - 1, drop_args(p, row_base=ROW_BASE + 1, row_dev=row_dev))
        assert torch.equal(pl1[:, :, c_off:c_off + c].contiguous().view(torch.int16), bits[:, hw:])


def test_dropout_entry_points_refuse_bad_arguments():
    lib = N.lib()
    B, hw, c = 1, 32, 64
    xd = torch.randn(B * hw, c, device=DEV)
    part, nck = gn_stats(lib, xd, B, hw, c)
    ga = torch.ones(c, device=DEV)
    pl = torch.zeros(2, B * hw, c, dtype=torch.bfloat16, device=DEV)
    sums = torch.zeros(B, lib.wd_gn_bwd_nchunk(hw), 2, c, device=DEV)
    dx = torch.zeros(B * hw, c, device=DEV)
    d = drop_args(0.1)
    for dd, cc in ((None, c), (C.byref(d), 66)):  # no wd_dropout; c % 4
        fwd = (xd.data_ptr(), c, B, hw, cc, 2, part.data_ptr(), nck, 2, ga.data_ptr(), ga.data_ptr(), 1e-5, 1, pl[0].data_ptr(),
               pl[1].data_ptr(), c, 0, None, None, dd)
        bwd = (xd.data_ptr(), c, xd.data_ptr(), c, 0, B, hw, cc, 2, part.data_ptr(), nck, 2, ga.data_ptr(), ga.data_ptr(), 0, 1e-5, 1,
               sums.data_ptr())
        assert lib.wd_gn_apply_dropout(*fwd, _st()) == N.WD_EINVAL
        assert lib.wd_gn_bwd_stats_dropout(*bwd, dd, _st()) == N.WD_EINVAL
        assert lib.wd_gn_bwd_apply_dropout(*bwd, dx.data_ptr(), c, 0, dd, _st()) == N.WD_EINVAL
        assert lib.wd_gn_bwd_fused_dropout(*bwd, dx.data_ptr(), c, 0, dd, _st()) == N.WD_EINVAL
    torch.cuda.synchronize()
    assert not bool(pl.float().any()) and not bool(dx.any())


# ------------------------------------------------------------------------------------------ 2. backward kernels
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("B,hw,c,silu", [(2, 32, 64, 0), (3, 256, 320, 1), (2, 512, 320, 1)])
def test_gn_bwd_dropout_equals_the_plain_kernels_on_a_premasked_gradient(B, hw, c, silu, p):
    """dz sits at columns [4, 4 + c) of a wider matrix and gamma / beta at offset 4 of longer vectors: the mask is indexed by the
    channel inside the norm, not by either offset."""
    lib = N.lib()
    g = torch.Generator().manual_seed(hw + c + silu)
    x = torch.randn(B * hw, c, generator=g) * 2 + 0.5
    off, ld = 4, c + 8
    dz = torch.randn(B * hw, ld, generator=g)
    gamma, beta = torch.randn(ld, generator=g), torch.randn(ld, generator=g)
    keep = R.keep_mask(SEED, ROW_BASE + ROW_BASE_DEV, B, hw, c, LAYER, p).reshape(B * hw, c)
    pre = dz.clone()
    pre[:, off:off + c] = torch.from_numpy(np.where(keep, dz[:, off:off + c].numpy() * R.scale(p), np.float32(0.0)))
    assert pre.dtype == torch.float32
    xd, dzd, pred, gd, bd = x.to(DEV), dz.to(DEV), pre.to(DEV), gamma.to(DEV), beta.to(DEV)
    part, nck = gn_stats(lib, xd, B, hw, c)
    nb = lib.wd_gn_bwd_nchunk(hw)
    cpg = c // 32
    row_dev = torch.tensor([ROW_BASE_DEV], dtype=torch.int64, device=DEV)
    d = drop_args(p, row_dev=row_dev)
    dr = C.byref(d)

    def common(grad):
        return (xd.data_ptr(), c, grad.data_ptr(), ld, off, B, hw, c, cpg, part.data_ptr(), nck, c // 32, gd.data_ptr(), bd.data_ptr(),
                off, 1e-5, silu)

    def two_pass(grad, tail, stats, apply, acc):
        sums = torch.full((B, nb, 2, c), float("nan"), device=DEV)
        dx = torch.ones(B * hw, c, device=DEV) if acc else torch.full((B * hw, c), float("nan"), device=DEV)
        N.check(stats(*common(grad), sums.data_ptr(), *tail, _st()), "bwd stats")
        N.check(apply(*common(grad), sums.data_ptr(), dx.data_ptr(), c, acc, *tail, _st()), "bwd apply")
        torch.cuda.synchronize()
        return sums.cpu(), dx.cpu()

    def one_pass(grad, tail, fused, acc):
        sums = torch.full((B, 1, 2, c), float("nan"), device=DEV)
        dx = torch.ones(B * hw, c, device=DEV) if acc else torch.full((B * hw, c), float("nan"), device=DEV)
        N.check(fused(*common(grad), sums.data_ptr(), dx.data_ptr(), c, acc, *tail, _st()), "bwd fused")
        torch.cuda.synchronize()
        return sums.cpu(), dx.cpu()

    for acc in (1, 0):
        s0, dx0 = two_pass(pred, (), lib.wd_gn_bwd_stats, lib.wd_gn_bwd_apply, acc)
        s1, dx1 = two_pass(dzd, (dr,), lib.wd_gn_bwd_stats_dropout, lib.wd_gn_bwd_apply_dropout, acc)
        assert bool(torch.isfinite(s0).all()) and bool(torch.isfinite(dx0).all())
        assert torch.equal(s1, s0), "two-pass sums"
        assert torch.equal(dx1, dx0), "two-pass dx"
    fused_ok = bool(lib.wd_gn_bwd_fused_supported(hw, c, cpg))
    assert fused_ok == (c % 40 == 0 and hw <= 448)
    if fused_ok:
        for acc in (1, 0):
            s0, dx0 = one_pass(pred, (), lib.wd_gn_bwd_fused, acc)
            s1, dx1 = one_pass(dzd, (dr,), lib.wd_gn_bwd_fused_dropout, acc)
            assert bool(torch.isfinite(s0).all()) and bool(torch.isfinite(dx0).all())
            assert torch.equal(s1, s0), "fused sums"
            assert torch.equal(dx1, dx0), "fused dx"


# ------------------------------------------------------------------------------------------ 3. / 4. model and TrainStep vs oracle
P_DROP = 0.1
_KEY = "out_layers.3.weight"


def oracle_layers(variant):
    """{prefix: layer} from the reference's state_dict layout alone."""
    keys = [k for k, _ in U.state_dict_shapes(FULL, variant) if k.endswith(_KEY)]
    return {k[: -len(_KEY)]: i for i, k in enumerate(keys)}


def dropped_resblock(layers, seed, row_base, p):
    """``U.resblock`` restated with the host mask on the post-SiLU activation of out_layers (unet.py:616-623: GroupNorm32, SiLU,
    Dropout(p), conv)."""
    def resblock(sd, pfx, x, emb):
        h = F.silu(U.group_norm(x, sd[pfx + "in_layers.0.weight"], sd[pfx + "in_layers.0.bias"], 1e-5))
        h = F.conv2d(h, sd[pfx + "in_layers.2.weight"], sd[pfx + "in_layers.2.bias"], padding=1)
        e = F.linear(F.silu(emb), sd[pfx + "emb_layers.1.weight"], sd[pfx + "emb_layers.1.bias"])
        h = h + e[:, :, None, None]
        h = F.silu(U.group_norm(h, sd[pfx + "out_layers.0.weight"], sd[pfx + "out_layers.0.bias"], 1e-5))
        B, c, hh, ww = h.shape
        keep = R.keep_mask(seed, row_base, B, hh * ww, c, layers[pfx], p).reshape(B, hh, ww, c)
        h = h * (torch.from_numpy(keep).permute(0, 3, 1, 2).to(h.dtype) * float(R.scale(p)))
        h = F.conv2d(h, sd[pfx + "out_layers.3.weight"], sd[pfx + "out_layers.3.bias"], padding=1)
        if pfx + "skip_connection.weight" in sd:
            w = sd[pfx + "skip_connection.weight"]
            x = F.conv2d(x, w, sd[pfx + "skip_connection.bias"], padding=w.shape[-1] // 2)
        return x + h
    return resblock


def case_inputs(B, hw, seeds, noised=False):
    inp = synthetic_inputs(B, seed=seeds[1], hw=hw, num_classes=FULL["num_classes"], phosc_len=0)
    eps = torch.from_numpy(np.random.RandomState(seeds[2]).standard_normal(tuple(inp["x"].shape)).astype(np.float32))
    x = inp["x"]
    if noised:
        x = D.noise_images(D.schedule(1000)[2], x, inp["t"], eps)
    return x, inp, eps


@functools.lru_cache(maxsize=2)
def reference64(variant, B, hw, seeds, drop_seed, row_base, noised=False):
    """float64 oracle (ResBlocks with the host dropout mask) -> MSE -> autograd: (pred, loss, {name: grad})."""
    x, inp, eps = case_inputs(B, hw, seeds, noised)
    sd = {k: torch.from_numpy(synthetic_tensor(k, s, seeds[0])).double().requires_grad_(True)
          for k, s in U.state_dict_shapes(FULL, variant)}
    orc = U.UNetOracle(FULL, sd, variant, False)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(U, "resblock", dropped_resblock(oracle_layers(variant), drop_seed, row_base, P_DROP))
        pred = orc(x.double(), inp["t"], inp["context"], inp["y"], None)
    loss = F.mse_loss(pred, eps.double())
    loss.backward()
    return pred.detach(), float(loss.detach()), {k: v.grad for k, v in sd.items() if v.grad is not None}


def check_against_reference(pred, loss, grads, ref, label):
    """The bounds of test_gpu_training.check_against_reference: per-sample prediction max_rel < 5e-5, loss 1e-5 relative, the same
    set of parameters with a gradient, every gradient within 2e-4 ||ref|| + 1e-7."""
    pred_ref, loss_ref, gref = ref
    pred = pred.detach().cpu().double()
    assert pred.shape == pred_ref.shape
    worst_pred = max(max_rel(pred[b], pred_ref[b]) for b in range(pred.shape[0]))
    assert worst_pred < 5e-5, worst_pred
    assert abs(loss - loss_ref) <= 1e-5 * abs(loss_ref), (loss, loss_ref)
    assert set(grads) == set(gref), sorted(set(grads) ^ set(gref))[:10]
    worst, bad = ("", 0.0), []
    for k, r in gref.items():
        g = grads[k].detach().cpu().double()
        assert tuple(g.shape) == tuple(r.shape), k
        err, rn = float((g - r).norm()), float(r.norm())
        if rn > 1e-6 and err / rn > worst[1]:
            worst = (k, err / rn)
        if not err < 2e-4 * rn + 1e-7:
            bad.append((k, err, rn))
    print(f"{label}: worst per-sample prediction error {worst_pred:.2e}, worst relative gradient error {worst[1]:.2e} ({worst[0]})")
    assert not bad, f"{len(bad)} gradients off the reference: {bad[:8]}"


def train_model(variant, seed, dropout=P_DROP):
    cls = UNetModel if variant == "base" else UNetModelPhosc
    m = cls(args=make_args(device=DEV), **FULL, dropout=dropout)
    fill_module_(m, seed)
    return m.to(DEV).train()


def model_call(m, variant, x, inp):
    kw = dict(timesteps=inp["t"].to(DEV), context=inp["context"].to(DEV), y=inp["y"].to(DEV))
    return m(x.to(DEV), **kw) if variant == "base" else m(x.to(DEV), None, **kw)


@pytest.mark.parametrize("variant,B,hw", [("base", 3, (8, 16)), ("base", 2, (8, 32)), ("phosc", 2, (8, 32))])
def test_dropout_model_gradients_against_the_oracle(variant, B, hw):
    seeds = (21, 200 + B, 4)
    x, inp, eps = case_inputs(B, hw, seeds)
    m = train_model(variant, seeds[0])
    assert m.set_dropout_state(seed=77, row_base=1000) is m
    pred = model_call(m, variant, x, inp)
    loss = torch.nn.MSELoss()(eps.to(DEV), pred)
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    check_against_reference(pred, float(loss.detach()), grads, reference64(variant, B, hw, seeds, 77, 1000),
                            f"dropout {P_DROP} FULL {variant} B={B} {hw}")
    assert m.train_engine.dropout_row_base == 1000 + B  # the next forward draws the next rows
    plan = list(m.train_engine._tplans.values())[0]
    nres = sum(1 for k in DO.layer_ids(m) if not k.startswith("res."))
    assert sum(fn.__name__ == "wd_gn_apply_dropout" for fn, _, _ in plan.step) == nres == len(plan.dropouts)
    assert sum(fn.__name__ in ("wd_gn_bwd_fused_dropout", "wd_gn_bwd_apply_dropout") for fn, _, _ in plan.bwd) == nres


def test_train_step_draws_a_new_mask_on_every_replay():
    from worddiffusion_amd.optim import FusedAdamW
    from worddiffusion_amd.training import TrainStep
    seeds, B, hw = (21, 202, 4), 2, (8, 16)
    x0, inp, eps = case_inputs(B, hw, seeds)
    m = train_model("base", seeds[0])
    opt = FusedAdamW(m.parameters(), lr=0.0)
    diff = Diffusion(noise_steps=1000, img_size=(64, 256), args=make_args(device=DEV))
    args = (x0.to(DEV), inp["context"].to(DEV), inp["y"].to(DEV))

    def run(step):
        loss = float(step(*args, t=inp["t"], noise=eps.to(DEV)).cpu())
        torch.cuda.synchronize()
        return step._P.out.cpu(), loss, {k: g.clone() for k, g in step.eng.grads().items()}

    step = TrainStep(m, diff, opt, seed=77, use_graph=True)
    first, second = run(step), run(step)
    assert step._graph is not None
    assert any(not torch.equal(second[2][k], g) for k, g in first[2].items()), "the replayed step drew the first step's mask"
    check_against_reference(*first, reference64("base", B, hw, seeds, 77, 0, noised=True), "TrainStep step 0 (rows 0..)")
    check_against_reference(*second, reference64("base", B, hw, seeds, 77, B, noised=True), f"TrainStep step 1 (rows {B}..)")
    again = run(TrainStep(m, diff, opt, seed=77, use_graph=True))
    assert set(again[2]) == set(first[2])
    for k, g in first[2].items():
        assert torch.equal(again[2][k], g), f"{k}: a fresh TrainStep with the same seed gave another gradient"
    assert torch.equal(again[0], first[0])


# ------------------------------------------------------------------------------------------ 5. modes
def test_eval_no_grad_and_the_plan_without_dropout():
    seeds = (21, 205, 4)
    x, inp, eps = case_inputs(2, (8, 16), seeds)
    m, m0 = train_model("base", seeds[0]), train_model("base", seeds[0], dropout=0)
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="eval"):
            model_call(m, "base", x, inp)
        a, b = model_call(m.eval(), "base", x, inp), model_call(m0.eval(), "base", x, inp)
        torch.cuda.synchronize()
        assert torch.equal(a, b)
        m0.train()
        c = model_call(m0, "base", x, inp)  # p == 0: train mode without autograd runs the inference engine, as before
        torch.cuda.synchronize()
        assert torch.equal(c, b)
    pred = model_call(m0, "base", x, inp)
    torch.nn.MSELoss()(eps.to(DEV), pred).backward()
    torch.cuda.synchronize()
    plan = list(m0.train_engine._tplans.values())[0]
    assert not plan.dropouts
    for fn, _, what in list(plan.step) + list(plan.bwd):
        assert "dropout" not in fn.__name__ and "dropout" not in what, (fn.__name__, what)
