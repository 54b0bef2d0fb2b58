"""Host side of the PHOSCnet recogniser: the float64 restatement and the numpy kernel specifications of tests/_phoscnet_ref.py
against the reference's recorded outputs (tests/golden/phoscnet.npz) and against torch on the CPU, the module's state_dict
layout, and every refusal of ``PHOSCnet``, ``WordVerifier`` and the driver's verification arguments.  No GPU."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _phoscnet_ref as R
from tests._common import load_golden, max_rel
from worddiffusion_amd import PHOSCnet, WordVerifier
from worddiffusion_amd import _native as N
from worddiffusion_amd import driver
from worddiffusion_amd.phoscnet import CONV_STACK, N_FEAT, N_PHOS, N_PHOC, TPP_LEVELS, conv_layers


@pytest.fixture(scope="module")
def golden(golden_dir):
    return load_golden(golden_dir, "phoscnet")


# ---- the golden file and the float64 restatement ---------------------------------------------------------------------------
def test_restatement_matches_the_reference_outputs(golden):
    """The golden is fp32 on the CPU: 1e-5 (max-norm relative) bounds the restatement, not the kernels."""
    x = torch.from_numpy(golden["images"]).float() / 255.0
    assert golden["images"].shape == (2, 3, 50, 250) and golden["images"].dtype == np.uint8
    out = R.network_f64(R.golden_state_dict(int(golden["seed"][0])), x, want_stats=True)
    for k in ("features", "phos_logits", "phoc_logits", "phos", "phoc"):
        assert out[k].shape == golden[k].shape and max_rel(out[k], golden[k]) < 1e-5, k
    assert golden["features"].shape == (2, N_FEAT) and golden["phos"].shape == (2, N_PHOS) and golden["phoc"].shape == (2, N_PHOC)
    stats = np.array(out["conv_stats"])
    assert stats.shape == golden["conv_stats"].shape == (13, 2)
    assert np.abs(stats - golden["conv_stats"]).max() < 1e-5 * np.abs(golden["conv_stats"]).max()


def test_golden_conditions(golden):
    """What makes the golden a test: logits wide enough that the sigmoid hides nothing, live ReLU outputs, features of unit scale."""
    assert float(golden["phoc_logits"].std()) >= 0.5
    assert float(golden["phos_logits"].std()) >= 0.5 and 0.2 < float((golden["phos"] > 0).mean()) < 0.8
    assert 0.5 < float(golden["features"].std()) < 2.0
    assert abs(float(golden["gain"][0]) - R.GAIN) < 1e-12
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "phoscnet.npz")) < 200_000


def test_weights_crc_and_state_dict_layout(golden):
    sd = R.golden_state_dict(int(golden["seed"][0]))
    assert R.weights_crc(sd) == int(golden["crc"][0])
    want = {str(k): tuple(int(v) for v in str(s).split(",")) for k, s in zip(golden["keys"], golden["shapes"])}
    assert want == dict(R.state_dict_shapes())
    net = PHOSCnet()
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == want and list(net.state_dict()) == [str(k) for k in golden["keys"]]
    net.load_state_dict(sd, strict=True)
    assert not net.training
    layers = conv_layers(net)
    assert [i for i, _, _ in layers] == list(R.CONV_KEYS) and [i for i, _, p in layers if p] == list(R.POOL_BEFORE)
    assert [(c.in_channels, c.out_channels) for _, c, _ in layers] == [c for c in CONV_STACK if c != "P"] == list(R.CONV_CH)
    assert TPP_LEVELS == R.LEVELS and N_FEAT == 512 * sum(TPP_LEVELS)


# ---- the numpy specifications against torch --------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(5, 7), (2, 2), (4, 6)])
def test_relu_pool_spec_is_max_pool2d(h, w):
    rs = np.random.RandomState(h * 10 + w)
    x = rs.standard_normal((2 * h * w, 8)).astype(np.float32)
    x.reshape(-1)[::5] = -0.0
    nchw = torch.from_numpy(x).reshape(2, h, w, 8).permute(0, 3, 1, 2)
    got = R.relu_pool_np(x, 2, h, w, 1)
    assert np.array_equal(got, torch.relu(nchw).permute(0, 2, 3, 1).reshape(-1, 8).numpy()) and not np.signbit(got).any()
    want = F.max_pool2d(torch.relu(nchw), (2, 2), stride=2).permute(0, 2, 3, 1).reshape(-1, 8).numpy()
    assert np.array_equal(R.relu_pool_np(x, 2, h, w, 2), want)


def test_split_spec_is_the_bf16_pair():
    x = (np.random.RandomState(0).standard_normal(4096) * 10).astype(np.float32)
    x[:3] = [0.0, 1.0 + 2.0 ** -12, 1.5]
    hi, lo = R.split_np(x)
    t = torch.from_numpy(x)
    thi = t.to(torch.bfloat16)
    tlo = (t - thi.float()).to(torch.bfloat16)
    assert np.array_equal(hi.view(np.int16), thi.view(torch.int16).numpy()) and np.array_equal(lo.view(np.int16), tlo.view(torch.int16).numpy())
    assert lo[1] != 0 and lo[2] == 0


@pytest.mark.parametrize("h,w", [(3, 62), (2, 4), (1, 5), (3, 9)])
def test_tpp_spec_is_the_padded_pooling(h, w):
    x = np.random.RandomState(w).standard_normal((2 * h * w, 16)).astype(np.float32)
    nchw = torch.from_numpy(x).reshape(2, h, w, 16).permute(0, 3, 1, 2)
    for levels in (R.LEVELS, (3, 1, 16, 2)):
        assert np.array_equal(R.tpp_np(x, 2, h, w, levels), R.tpp_torch(torch.relu(nchw), levels).numpy())
    assert not R.tpp_np(-np.abs(x) - 1, 2, h, w).any()


@pytest.mark.parametrize("hs,ws,h,w", [(64, 256, 50, 250), (7, 9, 5, 4), (5, 4, 7, 9), (6, 8, 6, 8)])
def test_resize_spec_against_float64_interpolate(hs, ws, h, w):
    x = np.random.RandomState(1).random_sample((2, 3, hs, ws)).astype(np.float32)
    want = F.interpolate(torch.from_numpy(x).double(), size=(h, w), mode="bilinear", align_corners=False).numpy()
    assert np.abs(R.resize_np(x, h, w).astype(np.float64) - want).max() < 1e-6
    assert np.array_equal(R.resize_np(x, h, w, bgr=True), R.resize_np(x[:, ::-1].copy(), h, w))
    if (hs, ws) == (h, w):
        assert np.array_equal(R.resize_np(x, h, w), x)


def test_finish_and_score_specs():
    rs = np.random.RandomState(2)
    phos, phoc = rs.standard_normal((3, 165)).astype(np.float32), rs.standard_normal((3, 604)).astype(np.float32) * 4
    out = R.finish_np(phos, phoc)
    want = torch.cat([torch.relu(torch.from_numpy(phos).double()), torch.sigmoid(torch.from_numpy(phoc).double())], 1).numpy()
    assert out.shape == (3, 769) and np.abs(out - want).max() < 1e-15
    table = (rs.random_sample((37, 769)) * (rs.random_sample((37, 769)) < 0.3)).astype(np.float32)
    pred = (table[[3, 30, 11]] * 1.5 + 0.05 * rs.standard_normal((3, 769))).astype(np.float32)
    scores, best, best_score, tsc = R.score_np(pred, table, None, [3, -1, 37])
    cos = torch.cosine_similarity(torch.from_numpy(pred).double()[:, None, :], torch.from_numpy(table).double()[None, :, :], dim=2)
    assert np.abs(scores.astype(np.float64) - cos.numpy()).max() < 1e-4
    assert np.abs(R.cosine_f64(pred, table).numpy() - cos.numpy()).max() < 1e-12
    assert best.tolist() == [3, 30, 11] and np.array_equal(best_score, scores[[0, 1, 2], best])
    assert tsc[0] == scores[0, 3] and np.isnan(tsc[1]) and np.isnan(tsc[2])


def test_first_maximum_rule():
    s = np.array([[0.1, 0.7, 0.7, 0.2], [0.5, 0.5, 0.5, 0.5], [0.0, 0.1, 0.2, 0.9]], dtype=np.float32)
    assert R.first_max(s).tolist() == [1, 0, 3]
    table = np.random.RandomState(3).random_sample((6, 40)).astype(np.float32)
    table[4] = table[1]
    assert R.score_np(table[[4]], table)[1].tolist() == [1]


# ---- the header -----------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_exported():
    lib = N.lib()
    for name in ("wd_relu_pool_planes", "wd_tpp_max", "wd_resize_bilinear", "wd_phosc_finish", "wd_phosc_score"):
        assert name in N.header_symbols() and getattr(lib, name).restype is not None
    assert N.DEFINES["WD_TPP_MAX_LEVELS"] == 8 and N.DEFINES["WD_TPP_MAX_BINS"] == 16


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_phoscnet_refusals():
    net = PHOSCnet()
    x = torch.zeros(1, 3, 50, 250)
    with pytest.raises(N.NativeError, match="MI355X"):
        net(x)                                                   # no CPU fallback
    with pytest.raises(NotImplementedError, match="eval"):
        net.train()(x)
    net.eval()
    with pytest.raises(NotImplementedError, match="backward"):
        net(x.clone().requires_grad_(True))
    for bad in (torch.zeros(3, 50, 250), torch.zeros(1, 1, 50, 250), torch.zeros(0, 3, 50, 250), torch.zeros(1, 3, 3, 250),
                torch.zeros(1, 3, 50, 3), torch.zeros(1, 3, 50, 250, dtype=torch.uint8)):
        for call in (net, net.features, net.phosc):
            with pytest.raises(ValueError):
                call(bad)
    with pytest.raises(RuntimeError):
        net.load_state_dict({k: v for k, v in list(net.state_dict().items())[1:]}, strict=True)


def test_word_verifier_refusals(golden_dir, tmp_path):
    csv = R.write_alphabet_csv(golden_dir, str(tmp_path / "Alphabet.csv"))
    net = PHOSCnet()
    with pytest.raises(TypeError):
        WordVerifier(torch.nn.Linear(2, 2), csv)
    with pytest.raises(ValueError, match="version"):
        WordVerifier(net, csv, version="xx")
    with pytest.raises(ValueError, match="size"):
        WordVerifier(net, csv, size=(3, 250))
    with pytest.raises(OSError):
        WordVerifier(net, str(tmp_path / "missing.csv"))
    v = WordVerifier(net, csv)
    assert v.size == (50, 250) and not v.bgr
    for bad in (torch.zeros(3, 50, 250), torch.zeros(1, 4, 50, 250), torch.zeros(1, 3, 50, 250, dtype=torch.int32)):
        with pytest.raises(ValueError):
            v.prepare(bad)
    with pytest.raises(N.NativeError, match="MI355X"):
        v.prepare(torch.zeros(1, 3, 64, 256))                    # the recogniser is on the CPU
    with pytest.raises(ValueError, match="2 images but 1 words"):
        v.score(torch.zeros(2, 3, 50, 250), ["one"])
    with pytest.raises(ValueError, match="min_score"):
        v.check(torch.zeros(1, 3, 50, 250), ["one"])
    with pytest.raises(ValueError, match="lexicon"):
        v._lexicon([])
    with pytest.raises(ValueError, match="lexicon"):
        v._lexicon(["ok", ""])


def _parse(argv):
    return driver.parse_args(["--gt_train", "gt.txt", "--save_path", "out"] + argv)[1]


def test_driver_verification_arguments(capsys):
    a = _parse([])
    assert a.verify is None and a.verify_tries == 1 and a.verify_min_score is None and a.verify_lexicon is None
    a = _parse(["--verify", "net.pt", "--alphabet_csv", "A.csv", "--verify_min_score", "0.5", "--verify_lexicon", "lex.txt",
                "--verify_tries", "3"])
    assert (a.verify, a.verify_min_score, a.verify_lexicon, a.verify_tries) == ("net.pt", 0.5, "lex.txt", 3)
    bad = [["--verify_min_score", "0.5"], ["--verify_lexicon", "lex.txt"], ["--verify_tries", "2"],      # without --verify
           ["--verify", "net.pt"],                                                                         # no alphabet
           ["--verify", "net.pt", "--alphabet_csv", "A.csv", "--verify_tries", "0"],
           ["--verify", "net.pt", "--alphabet_csv", "A.csv", "--style_pair", "0", "1"],
           ["--verify", "net.pt", "--alphabet_csv", "A.csv", "--attn_maps", "maps"],
           ["--verify", "net.pt", "--alphabet_csv", "A.csv", "--encode_images", "dir"]]
    for argv in bad:
        with pytest.raises(SystemExit):
            _parse(argv)
    capsys.readouterr()
    with pytest.raises(SystemExit):
        driver.parse_args(["--lines", "l.txt", "--save_path", "out", "--verify", "net.pt", "--alphabet_csv", "A.csv"])
    capsys.readouterr()
    # latents only: a ValueError before any device is touched
    with pytest.raises(ValueError, match="stable_dif_path"):
        driver.main(["--gt_train", "gt.txt", "--save_path", "out", "--verify", "net.pt", "--alphabet_csv", "A.csv"])


def test_regenerate_verification_refusals():
    rows, wr = [("w", "img", "word")], {"w": 0}
    with pytest.raises(ValueError, match="VAE"):
        driver.regenerate(None, None, rows, wr, None, vae=None, verifier=object())
    with pytest.raises(ValueError, match="attention"):
        driver.regenerate(None, None, rows, wr, None, vae=object(), verifier=object(), attention=True)
    with pytest.raises(ValueError, match="verify_tries"):
        driver.regenerate(None, None, rows, wr, None, vae=object(), verifier=object(), verify_tries=0)
    for kw in (dict(verify_min_score=0.5), dict(verify_lexicon=["a"]), dict(verify_tries=2), dict(verify_csv="v.csv")):
        with pytest.raises(ValueError, match="need a verifier"):
            driver.regenerate(None, None, rows, wr, None, **kw)
