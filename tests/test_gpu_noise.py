"""The device noise stream against its specification.  Every default sample (``noise=None``) and every default training step
takes its Gaussian noise from ``philox_normal4`` (csrc/wd_misc.hip); the other GPU tests inject their noise from the host, or
compare one Philox kernel with another.  Here what the kernels draw is compared with ``tests/_philox_ref.py``, a numpy
restatement of Philox4x32-10 + Box-Muller that shares nothing with the library (and is itself held to Random123's known-answer
vectors in tests/test_philox_host.py): (a) ``wd_randn``, (b) the edges of the uniform convention, (c) the key of the three step
kernels, (d) the keys the Python callers pass.

Tolerance of a device draw z = r * trig against the float64 value of the same uniforms:  |z_dev - z_ref| <= 16 * 2^-24 * r_ref.
With ``logf`` and ``sincosf`` within 4 ulp each (HIP documents less; the file is built without fast-math) r is within
4/2 + 1 ulp (half the relative error of the logarithm - at the radius' smallest value, u = 1 - 2^-24, the logarithm's
relative error is still its ulp error - plus the square root's and the product's rounding), the trig factor within 4 * 2^-24
absolute, the final product adds half an ulp: under 8 * 2^-24 * r in all; the bound is twice that.  Where r_ref = 0 the device
value must be 0 exactly.  A wrong counter word, key word, round constant or shift moves a draw by O(1).  Each case prints its
largest err / tol; DESIGN.md section 4 records the largest of all."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _philox_ref as P  # noqa: E402
from tests._common import SMALL, make_args, max_rel  # noqa: E402
from worddiffusion_amd import Diffusion, UNetModel  # noqa: E402
from worddiffusion_amd import _native as N  # noqa: E402
from worddiffusion_amd.synthetic import fill_module_, synthetic_inputs  # noqa: E402

DEV = "cuda:0"
TOL = 16.0 * 2.0 ** -24
# More float4 draws than the 2048 x 256 = 524 288 threads a launch is capped at, (batch, n_per_sample): 3 rows of 2^18 draws (the
# second grid-stride pass starts exactly at row 2) and 5 rows of 150 001 (it starts 74 285 draws into row 3).  12 MB each.
BIG = [(3, 4 * 2 ** 18), (5, 4 * 150001)]
TAIL_SEED = 1234
TAILS = [(13898544, (0, 1), "max"), (3896489, (0, 1), "zero"), (42670038, (2, 3), "max"), (4356836, (2, 3), "zero")]


def _st():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _ref(batch, n, seed, offset, tag):
    """(z, r) of the specification, computed once per key and never written to."""
    z, r = P.randn(batch, n, seed, offset, tag, with_r=True)
    z.setflags(write=False)
    r.setflags(write=False)
    return z, r


def _check(dev, ref, what):
    """dev: device tensor of draws; ref = (z, r).  Returns err / tol at its worst."""
    z, r = ref
    got = dev.detach().cpu().numpy().astype(np.float64).reshape(z.shape)
    assert np.isfinite(got).all(), what
    zero = r == 0.0
    assert (got[zero] == 0.0).all(), (what, "a draw of radius 0 is not 0")
    ratio = np.zeros_like(z)
    ratio[~zero] = np.abs(got - z)[~zero] / (TOL * r[~zero])
    worst = float(ratio.max())
    print(f"noise err/tol {what}: {worst:.4f}")
    if worst > 1.0:
        i = np.unravel_index(int(ratio.argmax()), z.shape)
        raise AssertionError(f"{what}: element {i} is {got[i]!r}, the specification says {z[i]!r} (radius {r[i]:.4f}); "
                             f"err/tol {worst:.3g}, {int((ratio > 1.0).sum())} of {z.size} elements out of tolerance")
    return worst


def _randn(batch, n, seed, offset, stream_id):
    out = torch.full((batch, n), float("nan"), device=DEV)
    N.check(N.lib().wd_randn(out.data_ptr(), batch, n, seed, offset, stream_id, _st()), "wd_randn")
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------------------ (a) wd_randn
@pytest.mark.parametrize("seed", [0, 1234, 2 ** 32 + 7, 2 ** 62 - 1])
@pytest.mark.parametrize("n", [4, 12, 1024])
def test_randn_equals_the_specification(n, seed):
    for stream_id in (0, 1, 2, 3):
        _check(_randn(3, n, seed, 5, stream_id), _ref(3, n, seed, 5, P.STREAM | stream_id), f"wd_randn n={n} seed={seed} id={stream_id}")


@pytest.mark.parametrize("seed", [1234, 2 ** 62 - 1])
def test_randn_rows_across_the_carry_into_the_high_sample_word(seed):
    off = 2 ** 32 - 2  # rows 0, 1 have sample >> 32 == 0, rows 2, 3 have 1
    _check(_randn(4, 12, seed, off, 2), _ref(4, 12, seed, off, P.STREAM | 2), f"wd_randn offset=2^32-2 seed={seed}")


@pytest.mark.parametrize("batch,n", BIG)
def test_randn_past_the_grid_cap(batch, n):
    assert 2048 * 256 < batch * n // 4 < 2 * 2048 * 256
    _check(_randn(batch, n, 1234, 5, 0), _ref(batch, n, 1234, 5, P.STREAM | 0), f"wd_randn {batch} x {n}")


def test_randn_every_key_word_is_live():
    base = _randn(3, 1024, 7, 5, 0)
    assert torch.equal(base, _randn(3, 1024, 7, 5, 0))
    assert not torch.equal(base, _randn(3, 1024, 7, 5, 1))              # stream id
    assert not torch.equal(base, _randn(3, 1024, 2 ** 32 + 7, 5, 0))    # high word of the seed
    assert not torch.equal(base, _randn(3, 1024, 7, 2 ** 32 + 5, 0))    # high word of the sample
    assert not torch.equal(base[0], base[1]) and not torch.equal(base[:, :4], base[:, 4:8])  # row, element counter


# ------------------------------------------------------------------------------------------------ (b) the tails
@pytest.mark.parametrize("sample,lanes,kind", TAILS)
def test_randn_at_the_edges_of_the_uniforms(sample, lanes, kind):
    """u = 2^-24 (the largest radius, sqrt(48 ln 2)) and u = 1 (radius 0) in either pair: finite, in tolerance, and 0 where the
    radius is 0 - a [0, 1) uniform would put log(0) = -inf there."""
    ref = _ref(1, 4, TAIL_SEED, sample, P.STREAM | 0)
    z, r = ref
    if kind == "zero":
        assert r[0, lanes[0]] == 0.0 and r[0, lanes[1]] == 0.0
    else:
        assert abs(r[0, lanes[0]] - np.sqrt(48 * np.log(2))) < 1e-12
    out = _randn(1, 4, TAIL_SEED, sample, 0)
    assert torch.isfinite(out).all(), out
    _check(out, ref, f"wd_randn tail sample={sample} ({kind})")
    if kind == "zero":
        assert float(out[0, lanes[0]]) == 0.0 and float(out[0, lanes[1]]) == 0.0


# ------------------------------------------------------------------------------------------------ (c) the step kernels
def _tables(T=1000):
    return torch.ones(T, device=DEV), torch.zeros(T, device=DEV)


def _ddpm_z(batch, n, t, seed, offset):
    """x = eps = 0, ca = 1, cb = 0, cs = 1: what wd_ddpm_step leaves in x is the z it drew."""
    ones, zeros = _tables()
    x, eps = torch.zeros(batch, n, device=DEV), torch.zeros(batch, n, device=DEV)
    t_dev = torch.tensor([t], dtype=torch.int32, device=DEV)
    N.check(N.lib().wd_ddpm_step(x.data_ptr(), eps.data_ptr(), batch, n, ones.data_ptr(), zeros.data_ptr(), ones.data_ptr(),
                                 t_dev.data_ptr(), None, seed, offset, _st()), "wd_ddpm_step")
    torch.cuda.synchronize()
    return x


def _cfg_z(batch, n, t, seed, offset):
    ones, zeros = _tables()
    x, first, second = (torch.zeros(batch, n, device=DEV) for _ in range(3))
    t_dev = torch.tensor([t], dtype=torch.int32, device=DEV)
    N.check(N.lib().wd_ddpm_step_cfg(x.data_ptr(), first.data_ptr(), second.data_ptr(), 3.0, None, batch, n, ones.data_ptr(),
                                     zeros.data_ptr(), ones.data_ptr(), t_dev.data_ptr(), None, seed, offset, _st()),
            "wd_ddpm_step_cfg")
    torch.cuda.synchronize()
    return x


def _ddim_z(batch, n, t, seed, offset, c5=1.0):
    """Tables (0, 0, 0, 0, c5) at step index 0: x = c5 * z, with the timestep read from t_dev."""
    zero, sig = torch.zeros(1, device=DEV), torch.full((1,), c5, device=DEV)
    x, eps = torch.zeros(batch, n, device=DEV), torch.zeros(batch, n, device=DEV)
    k_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    t_dev = torch.tensor([t], dtype=torch.int32, device=DEV)
    N.check(N.lib().wd_ddim_step(x.data_ptr(), eps.data_ptr(), None, 0.0, None, batch, n, zero.data_ptr(), zero.data_ptr(),
                                 zero.data_ptr(), zero.data_ptr(), sig.data_ptr(), k_dev.data_ptr(), t_dev.data_ptr(), None, seed,
                                 offset, _st()), "wd_ddim_step")
    torch.cuda.synchronize()
    return x


STEP_KERNELS = {"wd_ddpm_step": _ddpm_z, "wd_ddpm_step_cfg": _cfg_z, "wd_ddim_step": _ddim_z}


@pytest.mark.parametrize("kernel", sorted(STEP_KERNELS))
def test_step_kernel_key_is_seed_row_timestep_element(kernel):
    draw = STEP_KERNELS[kernel]
    got = {}
    for t in (2, 3, 500, 999):
        got[t] = draw(3, 128, t, 77, 6)
        _check(got[t], _ref(3, 128, 77, 6, t), f"{kernel} t={t}")
    assert not torch.equal(got[2], got[3])
    # the tag is the bare timestep: stream 0 of wd_randn (tag 0x80000000) at the same seed and rows is another draw
    assert not torch.equal(got[2], _randn(3, 128, 77, 6, 0))
    for t in (1, 0):
        if kernel == "wd_ddim_step":
            # the DDIM update has no "t > 1" rule of its own (include/wdiff_hip.h): it adds no noise where c5[k] == 0, and where
            # the caller's sigma is not 0 (eta > 0 keeps one at t = 1) it draws under the tag t like at any other timestep
            assert not draw(3, 128, t, 77, 6, c5=0.0).any(), t
            _check(draw(3, 128, t, 77, 6), _ref(3, 128, 77, 6, t), f"{kernel} t={t}")
        else:
            assert not draw(3, 128, t, 77, 6).any(), t  # train.py:229-232: no noise in the last update


@pytest.mark.parametrize("batch,n", BIG)
def test_ddpm_step_past_the_grid_cap(batch, n):
    _check(_ddpm_z(batch, n, 500, 77, 6), _ref(batch, n, 77, 6, 500), f"wd_ddpm_step {batch} x {n} t=500")


# ------------------------------------------------------------------------------------------------ (d) the callers
T_SMALL, ROWS, SEED, OFFSET = 12, 3, 99, 5
NPIX = 4 * 4 * 8


def _f32(a):
    return torch.from_numpy(a.astype(np.float32)).reshape(-1, 4, 4, 8)  # (astype copies: the cached reference stays untouched)


@pytest.fixture(scope="module")
def sampler():
    args = make_args(device=DEV)
    m = fill_module_(UNetModel(args=args, **SMALL), 5).to(DEV).eval()
    diff = Diffusion(noise_steps=T_SMALL, img_size=(32, 64), args=args)
    labels = torch.tensor([1, 7, 3], dtype=torch.int64)
    return m, diff, args, labels, ["MOVE", "a", "Zebra"]


def test_sampling_passes_seed_row_and_timestep(sampler):
    """Diffusion.sampling with device noise == the same call fed the specification's x_T (stream 0) and z_t (tag t, t = 11 .. 2),
    to the bar two 12-step runs that differ by rounding only are held to (test_sampling_device_noise_is_shard_invariant)."""
    m, diff, args, labels, words = sampler
    x_T = _f32(_ref(ROWS, NPIX, SEED, OFFSET, P.STREAM | 0)[0])
    noise = [_f32(_ref(ROWS, NPIX, SEED, OFFSET, t)[0]) for t in range(T_SMALL - 1, 1, -1)]
    want = diff.sampling(m, None, ROWS, words, labels, args, x_T=x_T, noise=noise)
    assert torch.isfinite(want).all() and float(want.std()) > 0.05
    for use_graph in (True, False):
        got = diff.sampling(m, None, ROWS, words, labels, args, seed=SEED, sample_offset=OFFSET, use_graph=use_graph)
        assert diff.last_stats["graph"] == use_graph
        err = max_rel(got.cpu(), want.cpu())
        print(f"sampling device noise vs specification noise (graph={use_graph}): max_rel {err:.2e}")
        assert err < 1e-5, (use_graph, err)
    # ... and the comparison can tell: with the draw of t = 7 also used at t = 8 the latent moves by sqrt(beta_8) * O(1), about
    # a tenth of its scale
    wrong = list(noise)
    wrong[3] = noise[4]
    assert max_rel(diff.sampling(m, None, ROWS, words, labels, args, x_T=x_T, noise=wrong).cpu(), want.cpu()) > 1e-3


def test_sampling_ddim_passes_the_visited_timestep(sampler):
    """eta = 1: every visited step draws, step k under the tag tau[k] (not k, and not a position in 11 .. 1)."""
    m, diff, args, labels, words = sampler
    tau = diff.ddim_timesteps(5)
    assert tau == [11, 8, 6, 3, 1]
    x_T = _f32(_ref(ROWS, NPIX, SEED, OFFSET, P.STREAM | 0)[0])
    noise = [_f32(_ref(ROWS, NPIX, SEED, OFFSET, t)[0]) for t in tau]
    want = diff.sampling_ddim(m, None, ROWS, words, labels, args, steps=5, eta=1.0, x_T=x_T, noise=noise)
    got = diff.sampling_ddim(m, None, ROWS, words, labels, args, steps=5, eta=1.0, seed=SEED, sample_offset=OFFSET)
    assert diff.last_stats["graph"] and diff.last_stats["timesteps"] == tau
    err = max_rel(got.cpu(), want.cpu())
    print(f"sampling_ddim device noise vs specification noise: max_rel {err:.2e}")
    assert err < 1e-5, err


def test_noise_images_draws_stream_1():
    diff = Diffusion(noise_steps=1000, img_size=(32, 64), args=make_args(device=DEV))
    x = torch.randn(5, 4, 4, 8, generator=torch.Generator().manual_seed(2)).to(DEV)
    t = torch.tensor([1, 250, 500, 750, 999], dtype=torch.int64)
    _, eps = diff.noise_images(x, t, seed=3)
    torch.cuda.synchronize()
    assert eps.shape == x.shape
    _check(eps, _ref(5, NPIX, 3, 0, P.STREAM | 1), "noise_images eps")


def test_train_step_draws_stream_2_at_the_global_row():
    """TrainStep without ``noise``: eps of step s is stream 2 at rows s * B .. s * B + B - 1 (world 1, rank 0) under the step's seed."""
    from worddiffusion_amd.optim import FusedAdamW
    from worddiffusion_amd.training import TrainStep
    B, seed = 4, 2 ** 32 + 3
    m = fill_module_(UNetModel(args=make_args(device=DEV), **SMALL), 7).to(DEV).train()
    opt = FusedAdamW(m.parameters(), lr=1e-4)
    diff = Diffusion(noise_steps=1000, img_size=(32, 64), args=make_args(device=DEV))
    step = TrainStep(m, diff, opt, seed=seed)
    inp = synthetic_inputs(B, seed=1, hw=(4, 8), num_classes=SMALL["num_classes"])
    x, c, y = inp["x"].to(DEV), inp["context"].to(DEV), inp["y"].to(DEV)
    drawn = []
    for s in (0, 1):
        assert step.step_index == s
        loss = step(x, c, y)
        torch.cuda.synchronize()
        assert np.isfinite(float(loss.cpu()))
        drawn.append(step._eps.clone())
        _check(drawn[s], _ref(B, NPIX, seed, s * B, P.STREAM | 2), f"TrainStep eps step {s}")
    assert not torch.equal(drawn[0], drawn[1])
