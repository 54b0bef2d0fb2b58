"""Writer-free guidance, host side: the writer-dropout specification (``tests/_labeldrop_ref.py``) against raw Philox draws, the
keying's edge cases, the oracle with the writer term per sample against what the reference's own modules computed
(``tests/golden/writer_free.npz``, ``tools/make_golden_writer_free.py``), the argument errors and the header.

The oracle bars are those of ``tests/test_oracle_golden.py``: 2e-5 for a forward, 5e-5 for the states of a trajectory."""
import os
import types

import numpy as np
import pytest
import torch

from oracle import ddpm_oracle as D
from oracle import unet_oracle as U
from tests import _labeldrop_ref as R
from tests import _philox_ref as PH
from tests._common import SMALL, load_golden, max_rel
from worddiffusion_amd import _native as N
from worddiffusion_amd import dropout as DO
from worddiffusion_amd.synthetic import synthetic_tensor


# ------------------------------------------------------------------------------------------------ 1. the draw
def test_labeldrop_ref_is_word_zero_of_one_philox_draw_per_row():
    for name, (seed, row_base, B, p) in R.DRAWS.items():
        keep = R.keep_mask(seed, row_base, B, p)
        assert keep.shape == (B,) and keep.dtype == bool
        for b in range(B):
            row = row_base + b
            w = PH.philox4x32_10(0, 0x80000005, row & 0xFFFFFFFF, row >> 32, seed & 0xFFFFFFFF, seed >> 32)
            assert bool(keep[b]) == (int(w[0]) >= int(p * 2.0 ** 32 + 0.5)), (name, b)
    assert list(R.y_eff([4, 5, 6], np.array([True, False, True]))) == [4, -1, 6]


def test_every_draw_the_gpu_tests_use_is_mixed():
    for name, (seed, row_base, B, p) in R.DRAWS.items():
        keep = R.keep_mask(seed, row_base, B, p)
        assert keep.any() and not keep.all(), f"{name}: {keep.astype(int)} tests nothing"
    # accumulation / sharding: two calls of B rows draw what one call of 2B rows draws
    for a, b, ab in (("step call 0", "step call 1", "step B=6"),):
        ma, mb, mab = (R.keep_mask(*R.DRAWS[k]) for k in (a, b, ab))
        assert np.array_equal(np.concatenate([ma, mb]), mab)


def test_threshold_and_tag_edge_cases():
    assert DO.threshold(0.0) == R.threshold(0.0) == 0
    assert R.keep_mask(3, 0, 64, 0.0).all()  # p = 0: every word >= 0
    for p in (0.1, 0.5, 0.999):
        assert DO.threshold(p) == R.threshold(p) == int(p * 2.0 ** 32 + 0.5) < 2 ** 32
    for bad in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError):
            DO.threshold(bad)
    kept = R.keep_mask(9, 0, 4096, 0.25).mean()
    assert abs(kept - 0.75) < 0.03
    tag = DO.label_tag()
    assert tag == R.label_tag() == 0x80000000 | N.DEFINES["WD_STREAM_LABEL_DROP"] == 0x80000005
    assert all(tag != DO.tag(layer) for layer in range(0, 4096))
    assert N.DEFINES["WD_STREAM_LABEL_DROP"] < N.STREAM_DROPOUT0
    assert N.DEFINES["WD_STREAM_LABEL_DROP"] not in (0, 1, 2, N.STREAM_VAE_POSTERIOR, N.STREAM_KNOWN)
    assert tag & 0x80000000 and not (N.TAG_KNOWN & 0x80000000)  # WD_TAG_KNOWN | p and the bare timesteps stay below 2^31
    with open(N.HEADER_PATH) as f:
        assert "#define WD_STREAM_LABEL_DROP 5" in f.read()


# ------------------------------------------------------------------------------------------------ 2. the oracle against the reference
def keep_oracle(variant, seed, dtype=torch.float32, cfg=SMALL, grad=False):
    sd = {k: torch.from_numpy(synthetic_tensor(k, s, seed)).to(dtype).requires_grad_(grad)
          for k, s in U.state_dict_shapes(cfg, variant)}
    return R.KeepOracle(cfg, sd, variant, False)


@pytest.mark.parametrize("tag", ["base", "phosc"])
def test_keep_oracle_reproduces_the_reference_forwards(golden_dir, tag):
    g = load_golden(golden_dir, "writer_free")
    orc = keep_oracle(tag, int(g[tag + "_seed"]))
    args = tuple(torch.from_numpy(g[tag + "_" + k]) for k in ("x", "t", "context", "y"))
    B = args[0].shape[0]
    with torch.no_grad():
        outs = {}
        for name, keep in (("cond", np.ones(B, bool)), ("free", np.zeros(B, bool)), ("plain", None)):
            orc.keep = keep
            outs[name] = orc(*args)
        orc.keep = np.array([True, False, True])
        mixed = orc(*args)
    for name in ("cond", "free"):
        err = max_rel(outs[name], g[f"{tag}_out_{name}"])
        print(f"writer-free oracle forward {tag} {name}: max_rel {err:.3e}")
        assert err < 2e-5, (tag, name)
    assert torch.equal(outs["plain"], outs["cond"])
    assert max_rel(outs["free"], g[tag + "_out_cond"]) > 1e-3  # the writer matters in this fixture
    for b, src in enumerate(("cond", "free", "cond")):  # samples are independent: each row follows its own decision
        assert max_rel(mixed[b], outs[src][b]) < 2e-5


def test_a_zeroed_label_table_is_the_imgconditioned_forward(golden_dir):
    """What justifies the PHOSC fixture, whose model has no imgConditioned flag: on the base model, where both exist, the
    reference's forward with ``label_emb.weight`` zeroed is its ``imgConditioned = 1`` forward."""
    g = load_golden(golden_dir, "writer_free")
    assert np.array_equal(g["base_out_zero"], g["base_out_free"])
    assert "phosc_out_zero" not in g.files


def oracle_trajectory(g, tag, variant, dtype=torch.float32):
    """The reference loop (train.py:221-236) on the oracle: per step the conditional forward, the writer-free one and
    ``torch.lerp(free, cond, s)``, replayed with the recorded start and noise."""
    T, s = int(g[tag + "_T"]), float(g[tag + "_cfg_scale"])
    n = g[tag + "_labels"].shape[0]
    orc = keep_oracle(variant, int(g[tag + "_seed"]), dtype)
    ctx = torch.tensor([D.label_padding(str(g[tag + "_word"]))] * n, dtype=torch.int64)
    y = torch.from_numpy(g[tag + "_labels"])
    noise = torch.from_numpy(g[tag + "_noise"]).to(dtype)
    preds, guided, rec = [], [], []

    def model(x, t):
        orc.keep = np.ones(n, bool)
        cond = orc(x, t, ctx, y)
        orc.keep = np.zeros(n, bool)
        free = orc(x, t, ctx, y)
        preds.extend([cond, free])
        guided.append(torch.lerp(free, cond, s))
        return guided[-1]

    with torch.no_grad():
        x0 = D.sampling(model, noise[0], list(noise[1:]), T, rec)
    return torch.stack(rec), torch.stack(preds), torch.stack(guided), x0


@pytest.mark.parametrize("tag,variant", [("gb3", "base"), ("gb025", "base"), ("gp3", "phosc"), ("gp025", "phosc")])
def test_keep_oracle_reproduces_the_reference_trajectories(golden_dir, tag, variant):
    g = load_golden(golden_dir, "writer_free")
    xs, preds, _, x0 = oracle_trajectory(g, tag, variant)
    assert preds.shape == tuple(g[tag + "_pred"].shape) and preds.shape[0] == 2 * (int(g[tag + "_T"]) - 1)
    ex, ep = max_rel(xs, g[tag + "_x_per_step"]), max(max_rel(p, q) for p, q in zip(preds, g[tag + "_pred"]))
    print(f"writer-free oracle trajectory {tag}: x max_rel {ex:.3e}, single predictions max_rel {ep:.3e}")
    assert ex < 5e-5 and ep < 2e-5, tag
    img = ((x0 / 0.18215) / 2 + 0.5).clamp(0, 1)
    assert float((img - torch.from_numpy(g[tag + "_image"])).abs().max()) < 2e-4
    # the two forwards of a step differ in this fixture: the guided prediction is not either of them
    assert max_rel(g[tag + "_pred"][1], g[tag + "_pred"][0]) > 1e-3


def test_golden_file_is_small(golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "writer_free.npz")) < 512 * 1024


# ------------------------------------------------------------------------------------------------ 3. arguments
def test_guidance_argument_errors():
    """``_guidance_setup`` is where a sampler decides; it needs no device."""
    from worddiffusion_amd import Diffusion
    diff = Diffusion(noise_steps=8)
    model = types.SimpleNamespace(interpolation=False, num_classes=11)
    assert diff._guidance_setup(model, None, 3, None) is None  # cfg_scale stays inert without the argument
    assert diff._guidance_setup(model, "writer_free", 3, None) == 3.0
    assert diff._guidance_setup(model, "writer_free", 0.25, None) == 0.25
    assert diff._guidance_setup(model, "writer_free", 0, None) is None  # train.py:223: one forward, the plain call
    for bad in ("writer", "text_free", True, 1):
        with pytest.raises(ValueError, match="guidance"):
            diff._guidance_setup(model, bad, 3, None)
    for bad in (-1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cfg_scale"):
            diff._guidance_setup(model, "writer_free", bad, None)
    with pytest.raises(ValueError, match="class-conditional"):
        diff._guidance_setup(types.SimpleNamespace(interpolation=False, num_classes=None), "writer_free", 3, None)
    # together with either interpolation mode: what _mix_setup returns for them is refused
    inter = types.SimpleNamespace(interpolation=True, num_classes=339)
    for mix in (diff._mix_setup(inter, 3, 0.37, None, 3), diff._mix_setup(model, 3, 0.5, (3, 7), 3)):
        assert mix is not None
        with pytest.raises(ValueError, match="interpolation"):
            diff._guidance_setup(inter, "writer_free", 3, mix)
    # a model built with args.interpolation but called without mix_rate does not interpolate (unet.py:1558): guidance runs
    assert diff._mix_setup(inter, 3, None, None, 3) is None
    assert diff._guidance_setup(inter, "writer_free", 3, None) == 3.0


def test_label_dropout_out_of_range_is_refused_before_any_device_work():
    from worddiffusion_amd.training import TrainStep
    for bad in (-0.1, 1.0, 2, float("nan")):
        with pytest.raises(ValueError, match="probability"):
            TrainStep(None, types.SimpleNamespace(noise_steps=8), None, label_dropout=bad)


def test_writer_keep_argument_is_checked_on_the_host():
    from worddiffusion_amd.engine import check_writer_keep
    assert check_writer_keep(torch.tensor([True, False, True]), 3).tolist() == [1, 0, 1]
    assert check_writer_keep(torch.tensor([2, 0], dtype=torch.uint8), 2).tolist() == [1, 0]
    assert check_writer_keep(np.array([True, False]), 2).dtype == torch.uint8
    for bad, B in ((torch.tensor([1.0, 0.0]), 2), (torch.tensor([1, 0]), 2), (torch.tensor([True]), 2), (True, 1)):
        with pytest.raises(ValueError, match="writer_keep"):
            check_writer_keep(bad, B)


def test_driver_guidance_arguments():
    from worddiffusion_amd import driver
    ap = driver.build_parser()
    a = ap.parse_args(["--gt_train", "g", "--save_path", "s", "--guidance", "writer_free", "--cfg_scale", "2.5"])
    assert a.guidance == "writer_free" and a.cfg_scale == 2.5
    a = ap.parse_args(["--gt_train", "g", "--save_path", "s"])
    assert a.guidance is None and a.cfg_scale == 3.0
    with pytest.raises(SystemExit):
        ap.parse_args(["--gt_train", "g", "--save_path", "s", "--guidance", "text_free"])
    with pytest.raises(ValueError, match="skip_steps"):
        driver.regenerate(None, None, [], {}, None, skip_steps=True, guidance="writer_free")


# ------------------------------------------------------------------------------------------------ 4. the C ABI
def test_writer_free_entry_points_are_declared_and_bound():
    names = ("wd_emb_combine_keep", "wd_label_rows_keep")
    assert set(names) <= set(N.header_symbols()) and set(names) <= set(N._SIGS)
    import ctypes as C
    sig = dict(N._PROTOS["wd_label_rows_keep"][1])
    assert sig["d"] == C.POINTER(N.WdDropout) and sig["keep_in"] is C.c_void_p and sig["y_eff"] is C.c_void_p
    if os.path.exists(N.LIB_PATH):
        lib = C.CDLL(N.LIB_PATH)
        for n in names:
            assert hasattr(lib, n), n
