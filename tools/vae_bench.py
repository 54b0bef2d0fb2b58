"""AutoencoderKL decode (default) or encode (--encode) of one batch at the reference's image size (for rocprofv3 --kernel-trace
--stats and timing).  Environment: B (batch, 64), PREC (bf16x3 | bf16), CHUNK (--encode: images per plan, the class default),
REPS (timed calls, 3)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from worddiffusion_amd import _native as N  # noqa: E402
from worddiffusion_amd.synthetic import fill_module_  # noqa: E402
from worddiffusion_amd.vae import AutoencoderKL  # noqa: E402

B = int(os.environ.get("B", "64"))
REPS = int(os.environ.get("REPS", "3"))
prec = os.environ.get("PREC", "bf16x3")
dev = "cuda:0"


def timed(fn, reps):
    """ms per call: events around ``reps`` calls after two warm-up calls (plans built, operands packed)."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, out


if "--encode" in sys.argv[1:]:
    vae = AutoencoderKL(with_encoder=True)
    fill_module_(vae, 0)
    vae = vae.to(dev).eval()
    vae.set_precision(prec)
    if "CHUNK" in os.environ:
        vae.encode_chunk = int(os.environ["CHUNK"])
    x = torch.rand(B, 3, 64, 256, device=dev) * 2 - 1
    ms, lat = timed(lambda: vae.encode_latents(x, seed=1), REPS)
    eng = vae.encoder_engine
    plans = {k[1]: eng.plan_bytes(P) for k, P in eng._plans.items()}
    print(f"vae encode B={B} {prec} chunk={vae.encode_chunk}: {ms:.2f} ms  finite={bool(torch.isfinite(lat).all())}  "
          f"plan bytes by batch {plans}")
    # the posterior kernel alone, on the moments of the last chunk: bytes moved = the token rows read + three NCHW maps written
    P = next(iter(eng._plans.values()))
    nb, L, (h, w) = P.x_in.shape[0], vae.config.latent_channels, P.lat_hw
    outs = [torch.empty(nb, L, h, w, device=dev) for _ in range(3)]
    st = torch.cuda.current_stream().cuda_stream

    def post():
        N.check(eng.lib.wd_vae_posterior(P.moments.data_ptr(), 2 * L, eng._w["qc.w"].data_ptr(), eng._w["qc.b"].data_ptr(), nb, L, h * w,
                                         outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), 0.18215, None, 1, 0, st), "posterior")
    pms, _ = timed(post, 200)
    nbytes = nb * h * w * (2 * L + 3 * L) * 4
    print(f"wd_vae_posterior batch {nb}: {pms * 1e3:.1f} us per launch (back to back), {nbytes} bytes, {nbytes / (pms * 1e-3) / 1e9:.1f} GB/s")
else:
    vae = AutoencoderKL()
    fill_module_(vae, 0)
    vae = vae.to(dev).eval()
    vae.set_precision(prec)
    z = torch.randn(B, 4, 8, 32, device=dev) / 0.18215
    ms, img = timed(lambda: vae.decode(z).sample, REPS)
    print(f"vae decode B={B}: {ms:.2f} ms  finite={bool(torch.isfinite(img).all())}")
