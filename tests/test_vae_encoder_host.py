"""Host-side pieces of the AutoencoderKL encoder: the right / bottom padded stride-2 gather table, the container's diffusers
layout, checkpoint loading, argument errors, the test's own float64 reference, the C exports and the latent-cache builder."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests._vae_encode_ref import vae_encode
from tests.test_host_logic import _gather_conv
from worddiffusion_amd import _native as N
from worddiffusion_amd.synthetic import fill_module_
from worddiffusion_amd.vae import AutoencoderKL

SMALL_VAE = dict(block_out_channels=(64, 128), layers_per_block=1)


@pytest.mark.parametrize("h,w", [(64, 256), (8, 32), (5, 7), (2, 3)])
def test_down_rb_table_equals_padded_stride2_conv(h, w):
    from worddiffusion_amd.engine import conv_gather_table
    g = torch.Generator().manual_seed(h * 100 + w)
    x = torch.randn(2, 6, h, w, generator=g)
    wt = torch.randn(5, 6, 3, 3, generator=g)
    b = torch.randn(5, generator=g)
    ref = F.conv2d(F.pad(x, (0, 1, 0, 1)), wt, b, stride=2)
    tab, ho, wo = conv_gather_table(h, w, "down_rb")
    assert (ho, wo) == ((h - 2) // 2 + 1, (w - 2) // 2 + 1) == tuple(ref.shape[2:])
    assert tab.shape == (9, ho * wo) and tab.dtype == np.int32 and tab.max() < h * w and tab.min() >= -1
    assert torch.allclose(_gather_conv(x, wt, b, "down_rb"), ref, atol=1e-5)
    if h % 2 == 0 and w % 2 == 0:  # same output size as the pad-1 table, different zero taps (left / top there)
        assert not np.array_equal(tab, conv_gather_table(h, w, "down")[0])


def test_encoder_state_dict_layout():
    m = AutoencoderKL(with_encoder=True)
    sd = m.state_dict()
    assert sum(v.numel() for k, v in sd.items() if k.startswith("encoder.")) == 34_163_592
    assert sum(v.numel() for k, v in sd.items() if k.startswith("quant_conv.")) == 72
    expect = {"encoder.conv_in.weight": (128, 3, 3, 3), "encoder.down_blocks.1.resnets.0.conv_shortcut.weight": (256, 128, 1, 1),
              "encoder.down_blocks.2.downsamplers.0.conv.weight": (512, 512, 3, 3),
              "encoder.mid_block.attentions.0.to_q.weight": (512, 512), "encoder.conv_out.weight": (8, 512, 3, 3),
              "quant_conv.weight": (8, 8, 1, 1)}
    for k, shp in expect.items():
        assert tuple(sd[k].shape) == shp, k
    assert not any("downsamplers" in k for k in sd if k.startswith("encoder.down_blocks.3."))
    assert any(k.startswith("encoder.down_blocks.3.resnets.1.") for k in sd)
    # the decoder half is the default object's, key for key, and the default object has nothing else
    d = AutoencoderKL().state_dict()
    assert all(k.startswith(("decoder.", "post_quant_conv.")) for k in d)
    assert list(d) == [k for k in sd if k.startswith(("decoder.", "post_quant_conv."))]
    assert all(d[k].shape == sd[k].shape for k in d)
    assert sum(v.numel() for k, v in d.items() if k.startswith("decoder.")) == 49_490_179
    assert set(sd) - set(d) == {k for k in sd if k.startswith(("encoder.", "quant_conv."))}
    # synthetic fills are keyed by name: the decoder's weights do not move when the encoder is added
    a, b = fill_module_(AutoencoderKL(**SMALL_VAE), 3), fill_module_(AutoencoderKL(with_encoder=True, **SMALL_VAE), 3)
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())


def _save(dirpath, model, old_names=False):
    from safetensors.torch import save_file
    dirpath.mkdir(parents=True)
    sd = {}
    for k, v in model.state_dict().items():
        if old_names:
            for new_n, old_n in (("to_q", "query"), ("to_k", "key"), ("to_v", "value"), ("to_out.0", "proj_attn")):
                if f"attentions.0.{new_n}." in k:
                    k = k.replace(f"attentions.0.{new_n}.", f"attentions.0.{old_n}.")
                    if v.dim() == 2:
                        v = v[:, :, None, None]
        sd[k] = v.contiguous()
    save_file(sd, str(dirpath / "diffusion_pytorch_model.safetensors"))
    (dirpath / "config.json").write_text(json.dumps({"block_out_channels": [64, 128], "layers_per_block": 1, "latent_channels": 4,
                                                     "_class_name": "AutoencoderKL"}))


@pytest.mark.parametrize("old_names", [False, True])
def test_from_pretrained_builds_the_encoder_the_checkpoint_holds(tmp_path, old_names):
    full = fill_module_(AutoencoderKL(with_encoder=True, **SMALL_VAE), 5)
    _save(tmp_path / "full" / "vae", full, old_names)
    back = AutoencoderKL.from_pretrained(str(tmp_path / "full"), subfolder="vae")
    assert back.with_encoder and set(back.state_dict()) == set(full.state_dict())
    for k, v in full.state_dict().items():
        assert torch.equal(v, back.state_dict()[k]), k
    assert not any(p.requires_grad for p in back.parameters())
    _save(tmp_path / "dec" / "vae", fill_module_(AutoencoderKL(**SMALL_VAE), 5), old_names)
    dec = AutoencoderKL.from_pretrained(str(tmp_path / "dec"), subfolder="vae")
    assert not dec.with_encoder and not hasattr(dec, "encoder") and not hasattr(dec, "quant_conv")
    # a decoder-only object still drops the encoder half of a full checkpoint, strictly
    AutoencoderKL(**SMALL_VAE).load_state_dict(full.state_dict())
    with pytest.raises(RuntimeError):
        AutoencoderKL(with_encoder=True, **SMALL_VAE).load_state_dict(AutoencoderKL(**SMALL_VAE).state_dict())


def test_encode_argument_errors():
    m = AutoencoderKL(with_encoder=True, **SMALL_VAE)
    with pytest.raises(N.NativeError):
        m.encode(torch.zeros(1, 3, 8, 16))              # CPU input
    with pytest.raises(ValueError):
        m.encode(torch.zeros(1, 4, 8, 16))              # wrong channel count
    with pytest.raises(ValueError):
        m.encode_latents(torch.zeros(1, 3, 7, 16))      # not a multiple of 2**(levels - 1)
    with pytest.raises(N.NativeError, match="with_encoder=True"):
        AutoencoderKL(**SMALL_VAE).encode(torch.zeros(1, 3, 8, 16))
    with pytest.raises(NotImplementedError):
        AutoencoderKL(with_encoder=True, latent_channels=N.VAE_MAX_LATENT + 1, **SMALL_VAE)
    assert m.encode_chunk == AutoencoderKL.ENCODE_CHUNK == 16


def test_float64_reference_agrees_with_itself_in_float32():
    cfg = dict(block_out_channels=(64, 64, 128), layers_per_block=1)
    m = fill_module_(AutoencoderKL(with_encoder=True, **cfg), 11)
    sd32 = m.state_dict()
    sd64 = {k: v.double() for k, v in sd32.items()}
    x = torch.rand(2, 3, 12, 20, generator=torch.Generator().manual_seed(1)) * 2 - 1
    m64, lv64 = vae_encode(sd64, x.double(), **cfg)
    m32, lv32 = vae_encode(sd32, x, **cfg)
    assert m64.shape == lv64.shape == (2, 4, 3, 5) and m64.dtype == torch.float64
    assert float(lv64.max()) <= 20.0 and float(lv64.min()) >= -30.0
    for a, b in ((m32, m64), (lv32, lv64)):
        assert float((a.double() - b).abs().max() / b.abs().max()) < 1e-4
    # the asymmetric padding matters: the symmetric stride-2 convolution is a different function
    k = "encoder.down_blocks.0.downsamplers.0.conv"
    h = torch.randn(1, 64, 6, 10, dtype=torch.float64)
    assert not torch.allclose(F.conv2d(F.pad(h, (0, 1, 0, 1)), sd64[k + ".weight"], sd64[k + ".bias"], stride=2),
                              F.conv2d(h, sd64[k + ".weight"], sd64[k + ".bias"], stride=2, padding=1))


def test_library_exports_the_posterior_kernels():
    assert os.path.exists(N.LIB_PATH), "build first: python -m worddiffusion_amd.build"
    lib = ctypes.CDLL(N.LIB_PATH)
    for sym in ("wd_vae_posterior", "wd_posterior_sample"):
        assert hasattr(lib, sym) and sym in N.header_symbols() and sym in N._SIGS
    hdr = open(N.HEADER_PATH).read()
    assert f"#define WD_VAE_MAX_LATENT {N.VAE_MAX_LATENT}" in hdr
    assert f"#define WD_STREAM_VAE_POSTERIOR {N.STREAM_VAE_POSTERIOR}" in hdr


class _StubVAE:
    """encode_latents as the real class, on the host: the latent of an image is its 8x8 block mean (+ the sample's offset when drawn)."""

    def __init__(self):
        self.calls = []

    def encode_latents(self, x, *, seed=None, sample_offset=0, mode=False):
        self.calls.append((x.shape[0], seed, sample_offset, mode))
        lat = F.avg_pool2d(x, 8).repeat(1, 2, 1, 1)[:, :4] * 0.18215
        if not mode:
            lat = lat + torch.arange(sample_offset, sample_offset + x.shape[0], dtype=torch.float32)[:, None, None, None]
        return lat


def test_build_latent_cache_with_a_stub_vae(tmp_path):
    from PIL import Image
    from worddiffusion_amd.latents import CachedLatentDataset, LatentCache, build_latent_cache, encode_images, load_image
    rs = np.random.RandomState(0)
    names = ["a01-000u-00-00", "a01-000u-00-01", "b02-111-03-07"]
    pix = {}
    for n in names:
        pix[n] = rs.randint(0, 256, size=(16, 32, 3)).astype(np.uint8)
        Image.fromarray(pix[n]).save(str(tmp_path / (n + ".png")))
    # PIL -> RGB -> ToTensor -> Normalize(0.5, 0.5)
    t = load_image(str(tmp_path / (names[0] + ".png")))
    assert t.shape == (3, 16, 32) and t.dtype == torch.float32
    assert torch.equal(t, (torch.from_numpy(pix[names[0]]).permute(2, 0, 1).float() / 255.0 - 0.5) / 0.5)
    rows = [("w1", names[0], "ab"), ("w2", names[1], "move"), ("w1", names[0], "ab"), ("w2", names[2], "To")]
    for mode in (True, False):
        vae = _StubVAE()
        out = build_latent_cache(vae, rows, str(tmp_path), str(tmp_path / f"lat{int(mode)}.safetensors"), mode=mode, seed=7, batch=2)
        cache = LatentCache(out)
        assert sorted(cache.keys()) == sorted(n + ".png" for n in names) and len(cache) == 3
        assert all(c[1] == 7 and c[3] == mode for c in vae.calls)
        for i, n in ((0, names[0]), (1, names[1]), (3, names[2])):   # the draw of a row is keyed by its index in ``rows``
            want = F.avg_pool2d(load_image(str(tmp_path / (n + ".png")))[None], 8).repeat(1, 2, 1, 1)[:, :4] * 0.18215
            want = want + (0.0 if mode else float(i))
            got = cache[n + ".png"]
            assert got.shape == (4, 2, 4) and torch.allclose(got, want[0], atol=1e-6)
        ds = CachedLatentDataset(rows, {"w1": 0, "w2": 1}, cache)
        b = next(ds.batches(4, shuffle=False, pin=False))
        assert b["latents"].shape == (4, 4, 2, 4) and torch.equal(b["latents"][0], b["latents"][2])
    # the batch size does not change which offsets the rows get
    v1, v2 = _StubVAE(), _StubVAE()
    a = LatentCache(build_latent_cache(v1, rows, str(tmp_path), str(tmp_path / "x1.safetensors"), seed=1, batch=1))
    b = LatentCache(build_latent_cache(v2, rows, str(tmp_path), str(tmp_path / "x2.npz"), seed=1, batch=64))
    assert all(torch.equal(a[k], b[k]) for k in a.keys())
    with pytest.raises(ValueError):
        encode_images(_StubVAE(), torch.zeros(1, 3, 8, 8, dtype=torch.int64), seed=0)
