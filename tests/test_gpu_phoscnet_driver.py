"""``regenerate(..., verifier=)`` and ``driver --verify``: a SMALL UNet, 2-step DDIM, a two-level VAE and the full-size PHOSCnet on
synthetic weights.  The two thresholds are derived in the test from direct scores of the very images the run decodes: one just
below the lowest (every row accepted at its first draw), one just above the highest of both draws (every row drawn twice,
nothing written).  Every ``verify.csv`` score equals a direct ``WordVerifier.score`` of the tensor the PNG is made from, the
redraw is the documented sample of the noise stream, and a run without a verifier writes the bytes the plain loop writes."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _phoscnet_ref as R  # noqa: E402
from tests._common import SMALL, make_args  # noqa: E402
from worddiffusion_amd import AutoencoderKL, Diffusion, PHOSCnet, UNetModel, WordVerifier  # noqa: E402
from worddiffusion_amd import driver  # noqa: E402
from worddiffusion_amd.synthetic import fill_module_  # noqa: E402

DEV = "cuda:0"
SEED, STEPS, T = 31, 2, 7


@pytest.fixture(scope="module")
def setup(golden_dir, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("verify")
    rows = driver.read_gt(os.path.join(golden_dir, "gt_samples.txt"))[:5]
    args = make_args(device=DEV)
    unet = fill_module_(UNetModel(args=args, **SMALL), 9).to(DEV).eval()
    vae = fill_module_(AutoencoderKL(block_out_channels=(64, 128), layers_per_block=1), 4).to(DEV).eval()
    net = PHOSCnet()
    net.load_state_dict(R.golden_state_dict())
    verifier = WordVerifier(net.to(DEV), R.write_alphabet_csv(golden_dir, str(tmp / "Alphabet.csv")))
    diff = Diffusion(noise_steps=T, img_size=(32, 64), args=args)
    return tmp, rows, args, unet, vae, verifier, diff


def _run(setup, out, **kw):
    tmp, rows, args, unet, vae, verifier, diff = setup
    return driver.regenerate(unet, diff, rows, driver.writer_dict(rows), args, vae=vae, batch=8, out_dir=str(out), seed=SEED, rank=0,
                             world=1, sampler="ddim", ddim_steps=STEPS, **kw)[1]


def _direct(setup, offset):
    """What the loop draws for all five rows at ``sample_offset = offset``."""
    tmp, rows, args, unet, vae, verifier, diff = setup
    words = [w for _, _, w in rows]
    labels = torch.tensor([driver.writer_dict(rows)[s] for s, _, _ in rows], dtype=torch.int64)
    return diff.sampling_ddim(unet, vae, len(rows), words, labels, args, steps=STEPS, eta=0.0, phoscLabels=None, seed=SEED,
                              sample_offset=offset, mix_rate=None).detach()


def _csv(path):
    lines = open(path).read().splitlines()
    assert lines[0] == "image,word,score,best_word,accepted,try"
    return [ln.split(",") for ln in lines[1:]]


def test_without_verifier_the_plain_loop_is_unchanged(setup, tmp_path):
    tmp, rows = setup[0], setup[1]
    res = _run(setup, tmp_path / "plain")
    want = _direct(setup, 0).cpu()
    assert torch.equal(res, want) and res.shape[:2] == (5, 3)
    for (_, image, _), item in zip(rows, want):
        arr = (item.clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).numpy()
        driver.write_png(str(tmp_path / "want.png"), arr)
        assert open(tmp_path / "plain" / f"{image}.png", "rb").read() == open(tmp_path / "want.png", "rb").read(), image
    assert sorted(os.listdir(tmp_path / "plain")) == sorted(r[1] + ".png" for r in rows)


def test_thresholds_accept_all_and_reject_all(setup, tmp_path):
    tmp, rows, args, unet, vae, verifier, diff = setup
    words = [w for _, _, w in rows]
    first, second = _direct(setup, 0), _direct(setup, len(rows))   # try 0: samples 0..4; try 1: samples 5..9 (r + 1 * len(rows))
    assert not torch.equal(first, second)
    s0, s1 = verifier.score(first, words).cpu(), verifier.score(second, words).cpu()
    lo, hi = float(s0.min()) - 1e-3, float(torch.cat([s0, s1]).max()) + 1e-3
    lex = sorted(set(words))
    # ---- just below the lowest: every row accepted at its first draw and written
    res = _run(setup, tmp_path / "lo", verifier=verifier, verify_min_score=lo, verify_tries=2, verify_csv=str(tmp_path / "lo.csv"))
    log = _csv(tmp_path / "lo.csv")
    assert [r[0] for r in log] == [r[1] for r in rows] and [r[1] for r in log] == words
    assert [float(r[2]) for r in log] == s0.tolist() and all(r[3:] == ["", "1", "0"] for r in log)
    assert torch.equal(res, first.cpu())
    assert sorted(os.listdir(tmp_path / "lo")) == sorted(r[1] + ".png" for r in rows)
    assert open(tmp_path / "lo" / f"{rows[2][1]}.png", "rb").read() == _png(first[2].cpu(), tmp_path)
    # ---- just above the highest: every row drawn twice (the documented samples), nothing written
    res = _run(setup, tmp_path / "hi", verifier=verifier, verify_min_score=hi, verify_lexicon=lex, verify_tries=2,
               verify_csv=str(tmp_path / "hi.csv"))
    log = _csv(tmp_path / "hi.csv")
    assert len(log) == 10 and [r[5] for r in log] == ["0"] * 5 + ["1"] * 5 and all(r[4] == "0" for r in log)
    assert [float(r[2]) for r in log] == s0.tolist() + s1.tolist()
    best0, best1 = verifier.recognise(first, lex)[0], verifier.recognise(second, lex)[0]
    assert [r[3] for r in log] == best0 + best1
    assert torch.equal(res, second.cpu()) and os.listdir(tmp_path / "hi") == []
    # ---- one draw only: the same first attempt, no second
    _run(setup, tmp_path / "one", verifier=verifier, verify_min_score=hi, verify_csv=str(tmp_path / "one.csv"))
    assert [float(r[2]) for r in _csv(tmp_path / "one.csv")] == s0.tolist() and os.listdir(tmp_path / "one") == []


def _png(item, tmp_path):
    arr = (item.clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).numpy()
    driver.write_png(str(tmp_path / "one_want.png"), arr)
    return open(tmp_path / "one_want.png", "rb").read()


def test_command_line_verify(setup, golden_dir, tmp_path, monkeypatch):
    """``--verify CKPT``: the checkpoint is loaded with ``strict=True`` and the run logs one attempt per row."""
    tmp = setup[0]
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    rows_txt = [ln for ln in open(os.path.join(golden_dir, "gt_samples.txt")).read().splitlines() if ln.strip()][:3]
    (tmp_path / "gt.txt").write_text("\n".join(rows_txt) + "\n")
    torch.save(R.golden_state_dict(), tmp_path / "phoscnet.pt")
    vdir = tmp_path / "sd" / "vae"
    os.makedirs(vdir)
    (vdir / "config.json").write_text(json.dumps(dict(block_out_channels=[64, 128], layers_per_block=1)))
    torch.save(fill_module_(AutoencoderKL(block_out_channels=(64, 128), layers_per_block=1), 4).state_dict(), vdir / "diffusion_pytorch_model.bin")
    out = tmp_path / "out"
    torch.manual_seed(0)   # (no --models_path: the UNet keeps its random initialisation)
    driver.main(["--gt_train", str(tmp_path / "gt.txt"), "--save_path", str(out), "--writer_dict", str(tmp_path / "writers.json"),
                 "--batch_size", "4", "--emb_dim", "64", "--num_heads", "2", "--noise_steps", str(T), "--sampler", "ddim",
                 "--ddim_steps", str(STEPS), "--seed", "5", "--stable_dif_path", str(tmp_path / "sd"), "--verify",
                 str(tmp_path / "phoscnet.pt"), "--alphabet_csv", str(tmp / "Alphabet.csv"), "--verify_min_score", "-1.0",
                 "--verify_tries", "2"])
    log = _csv(out / "verify.csv")
    assert len(log) == 3 and all(r[4:] == ["1", "0"] for r in log) and all(-1.0 <= float(r[2]) <= 1.0 for r in log)
    assert sorted(os.listdir(out / "images")) == sorted(r[0] + ".png" for r in log)
