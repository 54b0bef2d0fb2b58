"""AutoencoderKL encoder on the HIP path: the posterior kernels against float64, the encoder against the float64 restatement
in tests/_vae_encode_ref.py on the same synthetic weights (parity unpinned, as for the decoder: diffusers and real VAE weights
are absent offline), and the users of it (latent cache, driver flag, pixels -> one training step).

Bounds.  u = 2**-24 is the unit roundoff of fp32.
  * quant_conv output: K = 2L products, each rounded, summed left to right, bias last: K roundings of products and K additions
    on partial sums that are bounded by S = sum |w_k x_k| + |b|, so |error| <= gamma_{K+1} S ~ (K + 1) u S; with the rounding of
    the float64 value itself to fp32 (u S) the tests ask for (K + 2) u S (K = 8: 10 u S).  The clamp does not increase it.
  * the draw  s * (m + exp(0.5 lv) z):  0.5 lv is exact, expf is within 2 ulp = 4 u, the product, the sum and the scale add u each;
    an input error (dm, dl) moves it by |s| (dm + std |z| 0.5 dl (1 + dl)).  Bound: |s| (dm + std |z| (0.505 dl + 8 u) + 3 u (|m| + std |z|)).
  * encoder parity: max abs error over max abs reference below 1e-4, the decoder test's bound for this architecture family.
"""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
SMALL_VAE = dict(block_out_channels=(64, 128), layers_per_block=1)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from worddiffusion_amd import _native as N
    return N, N.lib()


def _posterior_case(B, L, hw, ld, seed):
    """Random moments whose logvar pre-activations reach far outside [-30, 20] on both sides (the first seed from ``seed`` on
    whose draw does: the inputs are a fixed function of the arguments)."""
    K = 2 * L
    while True:
        case = _posterior_draw(B, L, hw, ld, seed)
        if float(case[4][:, L:].max()) > 45 and float(case[4][:, L:].min()) < -45:
            return case
        seed += 1


def _posterior_draw(B, L, hw, ld, seed):
    g = torch.Generator().manual_seed(seed)
    K = 2 * L
    x = torch.randn(B * hw, ld, generator=g)
    x[::3] *= 25.0
    w = torch.randn(K, K, generator=g) / K ** 0.5
    b = torch.randn(K, generator=g) * 0.5
    z = torch.randn(B, L, hw, generator=g)
    x64, w64, b64 = x[:, :K].double(), w.double(), b.double()
    pre = (x64 @ w64.t() + b64).reshape(B, hw, K).permute(0, 2, 1)           # [B, 2L, hw]
    bound = ((x64.abs() @ w64.abs().t() + b64.abs()).reshape(B, hw, K).permute(0, 2, 1)) * (K + 2) * U
    return x, w, b, z, pre, bound


@pytest.mark.parametrize("B,L,hw,ld", [(3, 4, 32, 12), (2, 4, 15, 8), (2, 3, 8, 7), (1, 8, 64, 16)])
def test_vae_posterior_kernel_matches_float64(B, L, hw, ld):
    N, lib = _lib()
    x, w, b, z, pre, bound = _posterior_case(B, L, hw, ld, 100 * L + hw)
    assert float(pre[:, L:].max()) > 45 and float(pre[:, L:].min()) < -45      # the clamp is exercised on both sides
    mean64, lv64 = pre[:, :L], pre[:, L:].clamp(-30.0, 20.0)
    xd, wd, bd, zd = x.to(DEV), w.reshape(2 * L, 2 * L, 1, 1).contiguous().to(DEV), b.to(DEV), z.contiguous().to(DEV)
    mean, lv, smp = (torch.full((B, L, hw), 7.0, device=DEV) for _ in range(3))
    scale = 0.18215

    def run(sample, noise, seed=0, off=0, sc=scale):
        N.check(lib.wd_vae_posterior(xd.data_ptr(), ld, wd.data_ptr(), bd.data_ptr(), B, L, hw, mean.data_ptr(), lv.data_ptr(),
                                     sample.data_ptr() if sample is not None else None, sc,
                                     noise.data_ptr() if noise is not None else None, seed, off, _st()), "wd_vae_posterior")

    # sample == NULL: moments only, the sample buffer is not touched
    run(None, None)
    torch.cuda.synchronize()
    assert float(smp.min()) == 7.0 == float(smp.max())
    em, el = (mean.cpu().double() - mean64).abs(), (lv.cpu().double() - lv64).abs()
    print(f"posterior L={L} hw={hw}: mean err/bound {float((em / bound[:, :L]).max()):.3f}  logvar err/bound "
          f"{float((el / bound[:, L:]).max()):.3f}")
    assert bool((em <= bound[:, :L]).all()) and bool((el <= bound[:, L:]).all())
    assert float(lv.max()) == 20.0 and float(lv.min()) == -30.0
    m0, l0 = mean.clone(), lv.clone()
    # noise given, scale != 1
    run(smp, zd)
    torch.cuda.synchronize()
    assert torch.equal(mean, m0) and torch.equal(lv, l0)
    std64, az = torch.exp(0.5 * lv64), z.double().abs()
    ref = scale * (mean64 + std64 * z.double())
    sb = scale * (bound[:, :L] + std64 * az * (0.505 * bound[:, L:] + 8 * U) + 3 * U * (mean64.abs() + std64 * az))
    es = (smp.cpu().double() - ref).abs()
    print(f"  sample err/bound {float((es / sb).max()):.3f}")
    assert bool((es <= sb).all())
    with_noise = smp.clone()
    # Philox path: z is what wd_randn writes under the documented stream id, bit for bit
    seed, off = 1234567, 5
    zr = torch.empty(B, L, hw, device=DEV)
    N.check(lib.wd_randn(zr.data_ptr(), B, L * hw, seed, off, N.STREAM_VAE_POSTERIOR, _st()), "wd_randn")
    ph = torch.empty_like(smp)
    run(ph, None, seed, off)
    run(smp, zr)
    assert torch.equal(ph, smp) and not torch.equal(ph, with_noise)
    # ... and the documented operation order on the kernel's own moments (expf against torch.exp: a few ulp)
    t = scale * (m0 + torch.exp(0.5 * l0) * zr)
    tol = abs(scale) * 8 * U * (m0.abs() + torch.exp(0.5 * l0) * zr.abs())
    assert bool(((ph - t).abs() <= tol).all())
    # the stored-moments kernel makes the same draw
    ps = torch.empty_like(smp)
    N.check(lib.wd_posterior_sample(m0.data_ptr(), l0.data_ptr(), B, L * hw, ps.data_ptr(), scale, None, seed, off, _st()), "ps")
    assert torch.equal(ps, ph)
    N.check(lib.wd_posterior_sample(m0.data_ptr(), l0.data_ptr(), B, L * hw, ps.data_ptr(), scale, zd.data_ptr(), 0, 0, _st()), "ps")
    assert torch.equal(ps, with_noise)
    run(ph, None, seed, off, sc=1.0)
    assert not torch.equal(ps, ph)


def test_posterior_kernels_reject_bad_arguments():
    N, lib = _lib()
    B, L, hw = 2, 4, 16
    x = torch.zeros(B * hw, 8, device=DEV)
    w, b = torch.zeros(8, 8, device=DEV), torch.zeros(8, device=DEV)
    outs = [torch.full((B, L, hw), 3.0, device=DEV) for _ in range(4)]
    m, lv, s, z = (t.data_ptr() for t in outs)

    def post(x_=x.data_ptr(), ld=8, w_=w.data_ptr(), b_=b.data_ptr(), B_=B, L_=L, hw_=hw, m_=m, lv_=lv, s_=s, z_=None):
        return lib.wd_vae_posterior(x_, ld, w_, b_, B_, L_, hw_, m_, lv_, s_, 1.0, z_, 0, 0, _st())

    bad = [post(x_=None), post(w_=None), post(b_=None), post(m_=None), post(lv_=None), post(L_=0), post(L_=N.VAE_MAX_LATENT + 1),
           post(ld=7), post(B_=0), post(hw_=0), post(L_=3, hw_=5, ld=8), post(s_=None, z_=z), post(m_=m + 4), post(s_=s + 8),
           lib.wd_posterior_sample(None, lv, B, L * hw, s, 1.0, None, 0, 0, _st()),
           lib.wd_posterior_sample(m, None, B, L * hw, s, 1.0, None, 0, 0, _st()),
           lib.wd_posterior_sample(m, lv, B, L * hw, None, 1.0, None, 0, 0, _st()),
           lib.wd_posterior_sample(m, lv, 0, L * hw, s, 1.0, None, 0, 0, _st()),
           lib.wd_posterior_sample(m, lv, B, 6, s, 1.0, None, 0, 0, _st()),
           lib.wd_posterior_sample(m, lv, B, L * hw, s + 4, 1.0, None, 0, 0, _st())]
    assert all(rc == N.WD_EINVAL for rc in bad), bad
    torch.cuda.synchronize()
    assert all(float(t.min()) == 3.0 == float(t.max()) for t in outs)   # nothing was launched
    assert post() == N.WD_OK


def test_posterior_sample_is_keyed_by_seed_and_sample_index():
    N, lib = _lib()
    g = torch.Generator().manual_seed(2)
    mean, lv = torch.randn(3, 4, 8, 32, generator=g).to(DEV), (torch.randn(3, 4, 8, 32, generator=g) * 2).to(DEV)
    n = mean[0].numel()

    def draw(m_, l_, seed, off):
        out = torch.empty_like(m_)
        N.check(lib.wd_posterior_sample(m_.data_ptr(), l_.data_ptr(), m_.shape[0], n, out.data_ptr(), 1.0, None, seed, off, _st()), "ps")
        return out

    whole = draw(mean, lv, 11, 0)
    assert torch.equal(whole[1:2], draw(mean[1:2], lv[1:2], 11, 1))
    assert torch.equal(whole[2:3], draw(mean[2:3], lv[2:3], 11, 2))
    assert torch.equal(whole, draw(mean, lv, 11, 0))
    other = draw(mean, lv, 12, 0)
    assert not torch.equal(whole, other) and not torch.equal(whole[0], whole[1])
    z = (whole - mean) / torch.exp(0.5 * lv)
    assert abs(float(z.mean())) < 0.05 and abs(float(z.std()) - 1.0) < 0.05


def _pair(cfg, seed):
    from worddiffusion_amd.synthetic import fill_module_
    from worddiffusion_amd.vae import AutoencoderKL
    m = AutoencoderKL(with_encoder=True, **cfg)
    fill_module_(m, seed)
    sd = {k: v.double() for k, v in m.state_dict().items()}
    return m.to(DEV).eval(), sd


def _images(B, H, W, seed=5):
    return torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(seed)) * 2 - 1


@pytest.mark.parametrize("cfg,B,H,W", [
    (dict(block_out_channels=(64, 128), layers_per_block=1), 3, 32, 64),             # two levels, one shortcut, odd batch
    (dict(block_out_channels=(128, 256, 512, 512), layers_per_block=2), 2, 64, 256),  # the SD-v1.5 config at the reference's image size
    (dict(block_out_channels=(64, 64, 128), layers_per_block=1), 1, 12, 20),          # odd-ish sizes (no fused statistics)
])
def test_vae_encode_matches_float64_restatement(cfg, B, H, W):
    from tests._vae_encode_ref import kl, vae_encode
    m, sd = _pair(cfg, 11)
    x = _images(B, H, W)
    rm, rl = vae_encode(sd, x.double(), cfg["block_out_channels"], cfg["layers_per_block"])
    dist = m.encode(x.to(DEV)).latent_dist
    n = len(cfg["block_out_channels"]) - 1
    assert dist.mean.shape == dist.logvar.shape == (B, 4, H >> n, W >> n)
    em = float((dist.mean.cpu().double() - rm).abs().max() / rm.abs().max())
    el = float((dist.logvar.cpu().double() - rl).abs().max() / rl.abs().max())
    print(f"encode {cfg['block_out_channels']} B={B} {H}x{W}: mean {em:.3e}  logvar {el:.3e}")
    assert em < 1e-4, em
    assert el < 1e-4, el
    assert m.encode(x.to(DEV), return_dict=False)[0].mean.shape == rm.shape
    # a second call replays the plan with equal bits
    d2 = m.encode(x.to(DEV)).latent_dist
    assert torch.equal(dist.mean, d2.mean) and torch.equal(dist.logvar, d2.logvar)
    # accessors
    assert dist.mode() is dist.mean and dist.parameters.shape == (B, 8, H >> n, W >> n)
    assert torch.allclose(dist.std ** 2, dist.var, rtol=1e-5)
    m64, l64 = dist.mean.cpu().double(), dist.logvar.cpu().double()
    k64 = kl(m64, l64)
    ek = float(((dist.kl().cpu().double() - k64).abs() / k64.abs()).max())
    print(f"  kl rel err vs float64 of the same moments {ek:.3e} (one fp32 rounding: {2 * U:.3e})")
    assert ek <= 2 * U                       # summed in float64 on the device, rounded to fp32 once
    assert torch.allclose(dist.kl().cpu().double(), kl(rm, rl), rtol=1e-3)
    # an in-place weight update re-packs the operands: the moments move by the bias step (the logvar stays far from its clamp here)
    assert float(dist.logvar.abs().max()) < 19.0
    with torch.no_grad():
        m.quant_conv.bias.add_(0.25)
    d3 = m.encode(x.to(DEV)).latent_dist
    assert torch.allclose(d3.mean, dist.mean + 0.25, atol=1e-5) and torch.allclose(d3.logvar, dist.logvar + 0.25, atol=1e-5)


def test_encode_chunking_sampling_and_precision():
    m, sd = _pair(SMALL_VAE, 7)
    x = _images(5, 16, 32, seed=9).to(DEV)
    sf = m.config.scaling_factor
    assert m.encode_chunk == 16
    whole = m.encode(x).latent_dist
    lat = m.encode_latents(x, seed=21, sample_offset=3)
    # encode_latents = scaling_factor * sample, the draw inside the encoder's last launch
    assert torch.equal(lat, sf * whole.sample(seed=21, sample_offset=3))
    assert torch.equal(lat, whole.sample(seed=21, sample_offset=3, scale=sf))
    assert torch.equal(m.encode_latents(x, mode=True), sf * whole.mean)
    assert not torch.equal(lat, m.encode_latents(x, seed=22, sample_offset=3))
    assert not torch.equal(m.encode_latents(x), m.encode_latents(x))      # default seed: one draw from torch's generator per call
    g = torch.Generator().manual_seed(3)
    a = whole.sample(generator=g)
    g.manual_seed(3)
    assert torch.equal(a, whole.sample(g))
    zn = torch.randn(whole.mean.shape, generator=torch.Generator().manual_seed(1)).to(DEV)
    assert torch.allclose(m.encode_latents(x, noise=zn), sf * (whole.mean + whole.std * zn), rtol=1e-5, atol=1e-6)
    # chunked: 2 + 2 + 1 images over two plans
    m.encode_chunk = 2
    parts = m.encode(x).latent_dist
    assert len(m.encoder_engine._plans) == 3
    dm = float((parts.mean - whole.mean).abs().max() / whole.mean.abs().max())
    dl = float((parts.logvar - whole.logvar).abs().max() / whole.logvar.abs().max())
    print(f"chunked vs unchunked moments: mean {dm:.3e} logvar {dl:.3e}")
    assert dm < 1e-4 and dl < 1e-4
    # the noise does not see the chunking: the same stored moments drawn whole and in the chunks' pieces
    from worddiffusion_amd.vae import DiagonalGaussianDistribution as D
    s_whole = whole.sample(seed=5, sample_offset=10)
    pieces = [D(whole.mean[b0:b0 + 2], whole.logvar[b0:b0 + 2]).sample(seed=5, sample_offset=10 + b0) for b0 in (0, 2, 4)]
    assert torch.equal(s_whole, torch.cat(pieces))
    assert torch.equal(m.encode_latents(x, seed=5, sample_offset=10), parts.sample(seed=5, sample_offset=10, scale=sf))
    m.encode_chunk = 16
    # set_precision covers the encoder
    from tests._vae_encode_ref import vae_encode
    rm, _ = vae_encode(sd, x.cpu().double(), **SMALL_VAE)
    m.set_precision("bf16")
    low = m.encode(x).latent_dist.mean
    e1 = float((low.cpu().double() - rm).abs().max() / rm.abs().max())
    m.set_precision("bf16x3")
    assert torch.equal(m.encode(x).latent_dist.mean, whole.mean)
    print(f"bf16 single pass mean err {e1:.3e}")
    assert 1e-5 < e1 < 5e-2 and not torch.equal(low, whole.mean)


def test_default_object_and_decode_are_untouched():
    from worddiffusion_amd.synthetic import fill_module_
    from worddiffusion_amd.vae import AutoencoderKL
    keys = list(AutoencoderKL().state_dict())
    assert all(k.startswith(("decoder.", "post_quant_conv.")) for k in keys)
    a = fill_module_(AutoencoderKL(**SMALL_VAE), 4).to(DEV).eval()
    b = fill_module_(AutoencoderKL(with_encoder=True, **SMALL_VAE), 4).to(DEV).eval()
    z = (torch.randn(2, 4, 4, 8, generator=torch.Generator().manual_seed(5)) * 3.0).to(DEV)
    assert torch.equal(a.decode(z).sample, b.decode(z).sample)
    x = _images(2, 8, 16).to(DEV)
    rec = b.decode(b.encode(x).latent_dist.mode()).sample
    assert rec.shape == x.shape and torch.isfinite(rec).all()
    assert torch.equal(a.decode(z).sample, b.decode(z).sample)      # ... also after the encoder engine exists
    from worddiffusion_amd import _native as N
    with pytest.raises(N.NativeError):
        a.encode(x)
    with pytest.raises(N.NativeError):
        b.encode(x.cpu())
    with pytest.raises(ValueError):
        b.encode(torch.zeros(1, 4, 8, 16, device=DEV))


class _PixelDataset:
    """The shape of ``train.py:261``: pixel batches with word ids and writer ids."""

    def __init__(self, n, num_classes):
        rs = np.random.RandomState(3)
        self.images = _images(n, 8, 16, seed=2)
        self.words = torch.from_numpy(np.where(rs.rand(n, 10) < 0.6, rs.randint(1, 53, size=(n, 10)), 52).astype(np.int64))
        self.s_id = torch.from_numpy(rs.randint(0, num_classes, size=n).astype(np.int64))

    def batches(self, batch_size, shuffle=True, seed=0, epoch=0, rank=0, world=1):
        for b0 in range(0, len(self.images) - batch_size + 1, batch_size):
            sl = slice(b0, b0 + batch_size)
            yield dict(images=self.images[sl], words=self.words[sl], s_id=self.s_id[sl])


def test_pixels_to_one_training_step():
    from tests._common import SMALL, make_args
    from worddiffusion_amd import Diffusion, UNetModel
    from worddiffusion_amd.latents import encode_images, train_epoch
    from worddiffusion_amd.optim import FusedAdamW
    from worddiffusion_amd.synthetic import fill_module_
    from worddiffusion_amd.training import TrainStep
    vae, _ = _pair(SMALL_VAE, 4)
    unet = fill_module_(UNetModel(args=make_args(device=DEV), **SMALL), 31).to(DEV).train()
    step = TrainStep(unet, Diffusion(noise_steps=1000, img_size=(32, 64), args=make_args(device=DEV)),
                     FusedAdamW(unet.parameters(), lr=1e-4), seed=5)
    ds = _PixelDataset(8, SMALL["num_classes"])
    lat = encode_images(vae, ds.images[:4].to(DEV), seed=1, sample_offset=0)
    assert lat.shape == (4, 4, 4, 8)
    loss = step(lat, ds.words[:4].to(DEV), ds.s_id[:4].to(DEV))
    assert torch.isfinite(loss).all() and float(loss) > 0
    res = train_epoch(step, ds, 4, DEV, seed=3, vae=vae)
    assert res["batches"] == 2 and np.isfinite(res["mean_loss"])


def _write_checkpoint(root, model):
    from safetensors.torch import save_file
    d = root / "vae"
    d.mkdir(parents=True)
    save_file({k: v.detach().cpu().contiguous() for k, v in model.state_dict().items()}, str(d / "diffusion_pytorch_model.safetensors"))
    (d / "config.json").write_text(json.dumps({"block_out_channels": [64, 128], "layers_per_block": 1, "latent_channels": 4}))


def test_latent_cache_and_driver_flag(tmp_path):
    from PIL import Image
    from worddiffusion_amd import driver
    from worddiffusion_amd.latents import CachedLatentDataset, LatentCache, build_latent_cache, load_image
    vae, _ = _pair(SMALL_VAE, 4)
    rs = np.random.RandomState(1)
    names = ["a01-000u-00-00", "a01-000u-00-01", "b02-111-03-07"]
    (tmp_path / "img").mkdir()
    for n in names:
        Image.fromarray(rs.randint(0, 256, size=(8, 16, 3)).astype(np.uint8)).save(str(tmp_path / "img" / (n + ".png")))
    rows = [("w1", names[0], "ab"), ("w2", names[1], "move"), ("w1", names[2], "To")]
    x = torch.stack([load_image(str(tmp_path / "img" / (n + ".png"))) for n in names]).to(DEV)
    want_mode = vae.encode_latents(x, mode=True).cpu()
    want_draw = vae.encode_latents(x, seed=6, sample_offset=0).cpu()
    cache = LatentCache(build_latent_cache(vae, rows, str(tmp_path / "img"), str(tmp_path / "mode.safetensors"), mode=True, batch=3))
    for i, n in enumerate(names):
        assert torch.equal(cache[n + ".png"], want_mode[i])
    cache = LatentCache(build_latent_cache(vae, rows, str(tmp_path / "img"), str(tmp_path / "draw.safetensors"), seed=6, batch=3))
    for i, n in enumerate(names):
        assert torch.equal(cache[n + ".png"], want_draw[i])
    b = next(CachedLatentDataset(rows, {"w1": 0, "w2": 1}, cache).batches(3, shuffle=False, pin=False))
    assert torch.equal(b["latents"], want_draw)
    # the driver flag: gt file + image directory + a local diffusers-layout checkpoint -> the same container
    _write_checkpoint(tmp_path / "sd", vae)
    gt = tmp_path / "gt.txt"
    gt.write_text("".join(f"{s},{n} {t}\n" for s, n, t in rows))
    out = tmp_path / "driver.safetensors"
    driver.main(["--gt_train", str(gt), "--save_path", str(tmp_path / "out"), "--stable_dif_path", str(tmp_path / "sd"),
                 "--encode_images", str(tmp_path / "img"), "--latents_out", str(out), "--latent_mode", "mode", "--batch_size", "3"])
    got = LatentCache(str(out))
    assert sorted(got.keys()) == sorted(n + ".png" for n in names)
    for i, n in enumerate(names):
        assert torch.equal(got[n + ".png"], want_mode[i])
    with pytest.raises(SystemExit):
        driver.main(["--gt_train", str(gt), "--save_path", str(tmp_path / "out"), "--encode_images", str(tmp_path / "img")])
