"""Known-region conditioning and partial-noise starts, the host side (no GPU): the specification's own identities
(``tests/_known_ref.py``), the retained schedules of ``start``, every argument error of ``Diffusion._known_setup``, the
resolution of ``known_noise="auto"``, ``latent_mask_from_pixels``, the binding and the driver's command line."""
import numpy as np
import pytest
import torch

from tests import _known_ref as K
from tests import _philox_ref as P
from worddiffusion_amd import Diffusion, latent_mask_from_pixels
from worddiffusion_amd import _native as N

HW = (32, 64)  # latents [4, 4, 8]
SHAPE = (3, 4, 4, 8)


def _operands(seed=0, n=64):
    g = np.random.RandomState(seed)
    return tuple(g.standard_normal((3, n)).astype(np.float32) for _ in range(3))


# ------------------------------------------------------------------------------------------------ the specification
def test_spec_identities():
    x, x0, z = _operands()
    sa = np.linspace(1.0, 0.1, 8, dtype=np.float32)
    sb = np.sqrt(1 - sa * sa).astype(np.float32)
    for p in (1, 5, 7):
        kv = K.known_value(x0, p, sa, sb, z)
        assert np.array_equal(kv, (sa[p] * x0).astype(np.float32) + (sb[p] * z).astype(np.float32))
        assert np.array_equal(K.blend(x, x0, np.zeros_like(x), p, sa, sb, z), x)
        assert np.array_equal(K.blend(x, x0, np.ones_like(x), p, sa, sb, z), kv)
        half = K.blend(x, x0, np.full_like(x, 0.5), p, sa, sb, z)
        assert not np.array_equal(half, x) and not np.array_equal(half, kv)
        assert np.allclose(half, 0.5 * (x.astype(np.float64) + kv), rtol=0, atol=1e-6)
    # p == 0: the known latent itself, whatever the tables hold there, and z is not read
    assert np.array_equal(K.blend(x, x0, np.ones_like(x), 0, sa * 0, sb, None), x0)
    m = np.zeros_like(x)
    m[:, ::2] = 1.0
    out = K.blend(x, x0, m, 0, sa, sb, None)
    assert np.array_equal(out[:, ::2], x0[:, ::2]) and np.array_equal(out[:, 1::2], x[:, 1::2])
    # m == 0 keeps x's bits where arithmetic would not: a NaN payload, a negative zero under x + 0 * (kv - x) with kv = inf
    odd = x.copy()
    odd.view(np.uint32)[0, 0] = 0x7FC12345
    odd[0, 1] = -0.0
    inf = np.full_like(x0, np.inf)
    got = K.blend(odd, inf, np.zeros_like(x), 0, sa, sb, None)
    assert np.array_equal(got.view(np.uint32), odd.view(np.uint32))


def test_spec_predecessor_and_tags():
    assert [K.predecessor(t=t) for t in (7, 2, 1)] == [6, 1, 0]
    tau = [7, 5, 3, 1]
    assert [K.predecessor(k=k, tau=tau) for k in range(4)] == [5, 3, 1, 0]
    assert K.predecessor(k=0, tau=[7]) == 0
    # the three tag families are disjoint for every level of any schedule here (t, p < 2^30; stream ids < 2^30)
    assert K.TAG_KNOWN == N.TAG_KNOWN == 0x40000000 and K.STREAM_KNOWN == N.STREAM_KNOWN == 4 and P.STREAM == 0x80000000
    for p in (1, 999, 2 ** 30 - 1):
        assert (K.TAG_KNOWN | p) & P.STREAM == 0 and (K.TAG_KNOWN | p) >= 2 ** 30 > p
    a = K.draw(2, 8, 5, 3, 6)
    assert np.array_equal(a, P.randn(2, 8, 5, 3, 0x40000006))
    assert not np.array_equal(a, P.randn(2, 8, 5, 3, 6)) and not np.array_equal(a, K.draw(2, 8, 5, 3, 7))
    assert np.array_equal(K.draw(3, 8, 5, 2, 6)[1:], a)  # keyed by the global row
    assert np.array_equal(K.fixed_eps(2, 8, 5, 3), P.randn(2, 8, 5, 3, P.STREAM | 4))
    assert N.STREAM_KNOWN != N.STREAM_VAE_POSTERIOR and N.STREAM_KNOWN < N.STREAM_DROPOUT0


def test_symbol_is_declared_and_bound():
    assert "wd_known_blend" in N.header_symbols() and "wd_known_blend" in N._SIGS
    assert len(N._SIGS["wd_known_blend"][1]) == 15


# ------------------------------------------------------------------------------------------------ retained schedules
def _setup(d, start, tau=None, **kw):
    kw.setdefault("draws_noise", False)
    return d._known_setup(3, torch.zeros(SHAPE), None, start, "auto", tau=tau, **kw)


def test_start_retains_the_schedule_ddpm():
    T = 12
    d = Diffusion(noise_steps=T, img_size=HW)
    for start in (1, 5, T - 1):
        kn = _setup(d, start, draws_noise=True)
        assert (kn.start, kn.tau, kn.mask) == (start, None, None)
        s = d._ddpm(start=kn.start)
        assert [t for t, _, _ in s.steps] == list(range(start, 0, -1)) and all(f for _, f, _ in s.steps)
        assert [z for _, _, z in s.steps] == list(range(start - 1)) + [None]  # one ``noise`` entry per visited step with t > 1
        assert (s.t_first, s.tau, s.stats) == (start, None, dict(steps=start))
    full = d._ddpm()
    assert d._ddpm(start=T - 1).steps == full.steps and d._ddpm(start=T - 1).stats == full.stats
    for bad in (0, T, -3, 2.5, True, "7"):
        with pytest.raises((ValueError, TypeError)):
            _setup(d, bad, draws_noise=True)


@pytest.mark.parametrize("which", ["ddim", "dpmpp-time", "dpmpp-logsnr"])
def test_start_retains_the_schedule_of_the_subsequence_samplers(which):
    T, S = 40, 6
    d = Diffusion(noise_steps=T, img_size=HW)
    tau = d.ddim_timesteps(S) if which == "ddim" else d.dpmpp_timesteps(S, which.split("-")[1])
    assert len(tau) == S and tau[0] == T - 1 and tau[-1] == 1
    assert _setup(d, T - 1, tau).tau == tau and _setup(d, T - 1, tau).start == T - 1  # everything is retained
    kn = _setup(d, 1, tau)
    assert (kn.tau, kn.start) == ([1], 1)  # the last entry alone
    for start in (tau[2], tau[2] + 1, tau[3] + 1):  # on an entry, just above it, just above the next
        kn = _setup(d, start, tau)
        assert kn.tau == K.retained(tau, start) == [t for t in tau if t <= start] and kn.start == kn.tau[0] <= start
        assert kn.tau is not tau
    assert _setup(d, tau[2] - 1, tau).tau == tau[3:]
    # the samplers index their tables, FiLM rows and pairs by the retained list
    kn = _setup(d, tau[2], tau)
    s = d._ddim(kn.tau, 0.0) if which == "ddim" else d._dpmpp(kn.tau, 2)
    assert [row for row, _, _ in s.steps] == list(range(S - 2)) and (s.t_first, s.tau) == (tau[2], tau[2:])
    assert s.stats["steps"] == S - 2 and s.stats["timesteps"] == tau[2:]
    # a start below every entry leaves nothing to visit
    one = d.ddim_timesteps(1) if which == "ddim" else d.dpmpp_timesteps(1, which.split("-")[1])
    assert one == [T - 1]
    with pytest.raises(ValueError, match="below every visited timestep"):
        _setup(d, T - 2, one)
    with pytest.raises(ValueError, match="below every visited timestep"):
        _setup(d, 3, [30, 20, 4])
    for bad in (0, T):
        with pytest.raises(ValueError):
            _setup(d, bad, tau)


# ------------------------------------------------------------------------------------------------ arguments
def test_mask_shapes_expand_once_to_rows():
    d = Diffusion(noise_steps=8, img_size=HW)
    n, C, h, w = SHAPE
    g = torch.Generator().manual_seed(1)
    known = torch.randn(SHAPE, generator=g)
    for shape in ((h, w), (n, 1, h, w), SHAPE):
        m = torch.rand(shape, generator=g)
        kn = d._known_setup(n, known, m, None, "auto", draws_noise=True)
        assert kn.mask.shape == (n, C * h * w) and kn.mask.is_contiguous() and kn.mask.dtype == torch.float32
        assert torch.equal(kn.mask.reshape(SHAPE), m.expand(SHAPE))
        assert torch.equal(kn.x0.reshape(SHAPE), known) and kn.x0.is_contiguous() and (kn.start, kn.tau) == (None, None)
    b = d._known_setup(n, known.double(), torch.ones(h, w, dtype=torch.bool), None, "auto", draws_noise=True)
    assert b.x0.dtype == torch.float32 and bool((b.mask == 1).all())
    assert d._known_setup(n, None, draws_noise=True) is None  # nothing asked for: the call is what it always was


def test_every_argument_error():
    T = 8
    d = Diffusion(noise_steps=T, img_size=HW)
    n, C, h, w = SHAPE
    known, mask = torch.zeros(SHAPE), torch.ones(h, w)

    def bad(*a, **kw):
        kw.setdefault("draws_noise", True)
        with pytest.raises(ValueError):
            d._known_setup(n, *a, **kw)

    bad(None, mask)                                   # a mask without known
    bad(None, None, 3)                                # a start without known
    bad(None, None, None, "fixed")                    # a noise mode without known
    bad(known)                                        # known with nothing to do
    bad(torch.zeros(2, C, h, w), mask)                # n
    bad(torch.zeros(n, C, h, w + 1), mask)            # latent size
    bad(torch.zeros(n, C * h * w), mask)              # rank
    bad(torch.zeros(SHAPE, dtype=torch.int64), mask)  # dtype
    for shape in ((w, h), (1, 1, h, w), (n, h, w), (C, h, w), (n, 2, h, w), (h * w,)):
        bad(known, torch.ones(shape))
    bad(known, torch.ones(h, w, dtype=torch.int64))
    bad(known, mask * 1.5)
    bad(known, mask - 1.25)
    bad(known, torch.full((h, w), float("nan")))
    bad(known, mask, 3, x_T=torch.zeros(SHAPE))       # two starts
    bad(known, None, 3, x_T=torch.zeros(SHAPE))
    for s in (0, T, -1, 2.5):
        bad(known, mask, s)
    bad(known, mask, 3, tau=[7, 5])                   # nothing retained
    bad(known, mask, None, "repaint")
    bad(known, mask, None, torch.zeros(n, C, h, w + 1))
    bad(known, mask, None, torch.zeros(n, 1, h, w))
    bad(known, mask, None, torch.zeros(SHAPE, dtype=torch.int32))
    # x_T with a mask and no start is a start from the caller's latent, as ever
    assert d._known_setup(n, known, mask, None, "auto", torch.zeros(SHAPE), draws_noise=True).start is None


def test_samplers_refuse_on_the_host_before_any_device_work():
    """The public entry points validate first: on a machine without a GPU the argument error arrives, not the device's."""
    from tests._common import make_args
    d = Diffusion(noise_steps=8, img_size=HW)
    args = make_args(device="cpu")
    labels = torch.zeros(3, dtype=torch.int64)
    for call, kw in ((d.sampling, {}), (d.sampling_ddim, dict(steps=4)), (d.sampling_dpmpp, dict(steps=4))):
        with pytest.raises(ValueError):
            call(None, None, 3, "ab", labels, args, known_mask=torch.ones(4, 8), **kw)
        with pytest.raises(ValueError):
            call(None, None, 3, "ab", labels, args, known=torch.zeros(SHAPE), start=8, **kw)
        with pytest.raises(ValueError):
            call(None, None, 3, "ab", labels, args, known=torch.zeros(SHAPE), start=3, x_T=torch.zeros(SHAPE), **kw)
        with pytest.raises(N.NativeError):  # a valid call reaches the device check
            call(None, None, 3, "ab", labels, args, known=torch.zeros(SHAPE), start=3, **kw)
    with pytest.raises(ValueError):
        d.sampling_ddim(None, None, 3, "ab", labels, args, timesteps=[7, 5], known=torch.zeros(SHAPE), start=4)
    with pytest.raises(ValueError):  # ``noise`` holds one tensor per RETAINED step
        d.sampling_ddim(None, None, 3, "ab", labels, args, steps=4, eta=1.0, known=torch.zeros(SHAPE), start=4,
                        noise=[torch.zeros(SHAPE)] * 4)
    import inspect
    for name in ("sampling3", "sampling_modify_condition", "sampling_phosc"):  # the reference's signatures stay the reference's
        assert not {"known", "known_mask", "start", "known_noise"} & set(inspect.signature(getattr(Diffusion, name)).parameters)
    for name in ("sampling", "sampling_ddim", "sampling_dpmpp"):
        ps = inspect.signature(getattr(Diffusion, name)).parameters
        assert all(ps[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("known", "known_mask", "start", "known_noise"))
        assert ps["known_noise"].default == "auto" and ps["known"].default is None


def test_auto_resolves_by_whether_the_call_draws():
    d = Diffusion(noise_steps=8, img_size=HW)
    known, mask = torch.zeros(SHAPE), torch.ones(4, 8)
    mode = lambda kn, draws: d._known_setup(3, known, mask, None, kn, draws_noise=draws).mode  # noqa: E731
    assert mode("auto", True) == "fresh" and mode("auto", False) == "fixed"  # DDPM, DDIM eta > 0 | DDIM eta = 0, DPM++
    for draws in (True, False):
        assert mode("fresh", draws) == "fresh" and mode("fixed", draws) == "fixed"
        g = torch.randn(SHAPE, generator=torch.Generator().manual_seed(2))
        kn = d._known_setup(3, known, mask, None, g, draws_noise=draws)
        assert kn.mode == "fixed" and torch.equal(kn.eps.reshape(SHAPE), g) and kn.eps.shape == (3, 128)
        assert d._known_setup(3, known, mask, None, "fixed", draws_noise=draws).eps is None  # drawn on the device


# ------------------------------------------------------------------------------------------------ the pixel mask
def test_latent_mask_from_pixels_is_an_8x8_min_pool():
    px = np.ones((32, 64), dtype=bool)
    px[0, 0] = False      # one pixel of cell (0, 0)
    px[15, 63] = False    # the last pixel of cell (1, 7)
    px[16:24, 8:16] = False
    m = latent_mask_from_pixels(px)
    assert m.dtype == torch.float32 and m.shape == (4, 8)
    want = torch.ones(4, 8)
    want[0, 0] = want[1, 7] = want[2, 1] = 0
    assert torch.equal(m, want)
    f = latent_mask_from_pixels(torch.from_numpy(px).float() * 0.25)  # nonzero keeps
    assert torch.equal(f, want)
    b = latent_mask_from_pixels(torch.ones(2, 1, 64, 256))
    assert b.shape == (2, 1, 8, 32) and bool((b == 1).all())
    assert not latent_mask_from_pixels(torch.zeros(8, 8)).any()
    for shape in ((31, 64), (32, 60), (64,), (0, 8)):
        with pytest.raises(ValueError):
            latent_mask_from_pixels(torch.ones(shape))
    # what it returns is a mask the samplers take
    d = Diffusion(noise_steps=8, img_size=HW)
    assert torch.equal(d._known_setup(3, torch.zeros(SHAPE), m, None, "auto", draws_noise=True).mask.reshape(SHAPE), want.expand(SHAPE))


# ------------------------------------------------------------------------------------------------ the driver
def test_driver_command_line_and_regenerate_arguments():
    from worddiffusion_amd import driver
    base = ["--gt_train", "gt.txt", "--save_path", "out"]
    _, a = driver.parse_args(base)
    assert (a.init_latents, a.keep_cols, a.start) == (None, None, None)
    _, a = driver.parse_args(base + ["--init_latents", "c.npz", "--keep_cols", "0:12", "--start", "600", "--sampler", "ddim"])
    assert (a.init_latents, a.keep_cols, a.start) == ("c.npz", (0, 12), 600)
    _, a = driver.parse_args(base + ["--init_latents", "c.npz", "--keep_cols", "31:32"])
    assert a.keep_cols == (31, 32) and a.start is None
    for bad in (["--keep_cols", "0:12"], ["--start", "5"],                                  # no latents to start from
                ["--init_latents", "c.npz"],                                               # nothing to do with them
                ["--init_latents", "c.npz", "--keep_cols", "0:12", "--skip_steps", "1"],
                ["--init_latents", "c.npz", "--start", "5", "--skip_steps", "1"],
                ["--keep_cols", "0:12", "--skip_steps", "1"], ["--start", "5", "--skip_steps", "1"],
                ["--init_latents", "c.npz", "--keep_cols", "12"], ["--init_latents", "c.npz", "--keep_cols", "a:b"],
                ["--init_latents", "c.npz", "--keep_cols", "5:5"], ["--init_latents", "c.npz", "--keep_cols", "8:4"],
                ["--init_latents", "c.npz", "--keep_cols", "0:33"], ["--init_latents", "c.npz", "--keep_cols", "-1:4"],
                ["--init_latents", "c.npz", "--start", "0"], ["--init_latents", "c.npz", "--start", "1000"],
                ["--init_latents", "c.npz", "--start", "9", "--noise_steps", "9"],
                ["--init_latents", "c.npz", "--start", "5", "--style_pair", "1", "2"]):
        with pytest.raises(SystemExit):
            driver.parse_args(base + bad)
    m = driver.keep_cols_mask((2, 5), 4, 8)
    assert m.shape == (4, 8) and m.dtype == torch.float32 and bool((m[:, 2:5] == 1).all()) and float(m.sum()) == 12
    for bad in ((5, 5), (6, 2), (0, 9), (-1, 3), (1,), "ab", None):
        with pytest.raises(ValueError):
            driver.keep_cols_mask(bad, 4, 8)
    rows = [("w1", "img_a", "word"), ("w2", "img_b", "text")]
    d = Diffusion(noise_steps=8, img_size=HW)
    cache = {"img_a.png": torch.zeros(4, 4, 8)}
    for kw in (dict(keep_cols=(0, 2)), dict(start=3), dict(known=cache), dict(known=cache, keep_cols=(0, 2), skip_steps=True),
               dict(known=cache, keep_cols=(0, 9))):
        with pytest.raises(ValueError):
            driver.regenerate(None, d, rows, {"w1": 0, "w2": 1}, None, rank=0, world=1, **kw)
    with pytest.raises(KeyError, match="img_b"):  # the missing row is named, before anything is sampled
        driver.regenerate(None, d, rows, {"w1": 0, "w2": 1}, None, rank=0, world=1, known=cache, keep_cols=(0, 2))
