"""Line sampling (``windows=``) on the GPU: ``wd_window_gather`` / ``wd_window_blend`` against their host specification
(``tests/_window_ref.py``) bit for bit on guarded operands, their argument checks, and the three samplers around them - K = 1 is the
plain call, disjoint windows are independent samples, every step of a masked line call replayed through the C-ABI, graph replay
against eager launches, one float64 trajectory, sharding by the global line, the PHOSC model, refusals and the driver.

Bounds: equality of bits wherever two fp32 evaluations of the same expression are compared; 1e-4 max-norm relative for the
float64 trajectory, the bar ``tests/test_gpu_ddim.py`` holds its own float64 trajectory to (the blend is a convex combination of
the window predictions and adds one rounding per term, far below that bar).

One layout of the kernel test is kept as it was first written down, (c, h, w, wl, K) = (4, 8, 8, 20, 3) with offsets 0, 3, 12: its
column 11 is covered by no window (and none is covered three times, which 20 columns leave no room for).  The kernels and the
specification both leave 0.0 there; the test compares that layout on its covered columns.  (4, 8, 8, 14, 3) with offsets 0, 3, 6
is the layout that does cover columns three times."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ddpm_oracle as D  # noqa: E402
from oracle import unet_oracle as U  # noqa: E402
from tests import _ddim_ref as R  # noqa: E402
from tests import _guard as G  # noqa: E402
from tests import _window_ref as W  # noqa: E402
from tests._common import SMALL, make_args, max_rel  # noqa: E402
from worddiffusion_amd import Diffusion, UNetModel, UNetModelPhosc  # noqa: E402
from worddiffusion_amd import _native as N  # noqa: E402
from worddiffusion_amd.synthetic import fill_module_, synthetic_tensor  # noqa: E402

DEV = "cuda:0"
HW = (64, 64)
C, H, WM = 4, 8, 8  # the latent of HW
T = 8
SAMPLERS = ["ddpm", "ddim", "dpmpp"]


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _i32(*v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _gather(line, off, dims, win):
    return N.lib().wd_window_gather(_ptr(line), _ptr(off), *dims, _ptr(win), _st())


def _blend(win0, win1, wn, off, dims, line0, line1):
    return N.lib().wd_window_blend(_ptr(win0), _ptr(win1), _ptr(wn), _ptr(off), *dims, _ptr(line0), _ptr(line1), _st())


# ------------------------------------------------------------------------------------------------ 1. kernels against the specification
# name -> (c, h, w, wl, K, the offsets of lines 0, 1, 2)
LAYOUTS = {
    "one": (4, 8, 8, 8, 1, [[0]] * 3),
    "two": (4, 8, 8, 14, 2, [[0, 6]] * 3),
    "three-0-3-12": (4, 8, 8, 20, 3, [[0, 3, 12]] * 3),            # column 11 uncovered (module docstring)
    "three-0-6-12": (4, 8, 8, 20, 3, [[0, 6, 12], [0, 4, 12], [0, 8, 12]]),
    "three-deep": (4, 8, 8, 14, 3, [[0, 3, 6], [0, 2, 6], [0, 5, 6]]),  # columns covered three times
    "ragged": (4, 6, 26, 45, 2, [[0, 19]] * 3),                       # nothing a multiple of 4
    "workload": (4, 8, 32, 92, 3, [[0, 30, 60], [0, 28, 60], [0, 32, 60]]),
}
WEIGHTS = ["flat", "feather", "random"]


def _weights(kind, lines, K, w, g):
    if kind == "flat":
        return np.ones((lines, K, w), dtype=np.float32)
    if kind == "feather":
        return np.broadcast_to(W.profile(w, min(3, (w - 1) // 2)), (lines, K, w)).copy()
    return (0.1 + 0.9 * torch.rand(lines, K, w, generator=g)).numpy()


def _guarded(values):
    """(buf, view) with the values in a NaN-guarded window, on the device."""
    buf, view = G.guarded_flat(values.numel(), torch.float32, device=DEV)
    view.copy_(values.reshape(-1))
    return buf, view


def _check_layout(c, h, w, wl, K, off, wt, g, nan_window=None):
    """Gather and both forms of blend for one layout against the specification; ``nan_window``: a window whose predictions are NaN."""
    lines = off.shape[0]
    dims = (lines, K, c, h, w, wl)
    off_dev = torch.from_numpy(off.astype(np.int32)).to(DEV)
    wn = W.normalise(off, wt, wl, lines)
    cover = W.coverage(off, wt, wl, lines) > 0
    wn_dev = torch.from_numpy(wn).to(DEV)
    # gather
    line = torch.randn(lines, c, h, wl, generator=g)
    line[0, 0, 0, 0] = -0.0
    lbuf, lview = _guarded(line)
    wbuf, wview = G.guarded_flat(lines * K * c * h * w, torch.float32, device=DEV)
    assert _gather(lview, off_dev, dims, wview) == N.WD_OK
    torch.cuda.synchronize()
    G.assert_untouched(lbuf, lview, "line")
    G.assert_untouched(wbuf, wview, "win")
    assert torch.equal(lview.cpu(), line.reshape(-1)), "line was written"
    assert _same_bits(wview.reshape(lines * K, c, h, w), torch.from_numpy(W.gather(line.numpy(), off, w)))
    # blend, one prediction and two
    e0, e1 = (torch.randn(lines * K, c, h, w, generator=g) for _ in range(2))
    e0[0, 0, 0, 0] = -0.0
    if nan_window is not None:
        e0.reshape(lines, K, c, h, w)[:, nan_window] = float("nan")
        e1.reshape(lines, K, c, h, w)[:, nan_window] = float("nan")
    want0, want1 = (torch.from_numpy(W.blend(e.numpy(), wn, off, wl)) for e in (e0, e1))
    keep = torch.from_numpy(cover)[:, None, None, :].expand(lines, c, h, wl)
    (b0, v0), (b1, v1) = _guarded(e0), _guarded(e1)
    outs = []
    for two in (False, True):
        (o0buf, o0), (o1buf, o1) = (G.guarded_flat(lines * c * h * wl, torch.float32, device=DEV) for _ in range(2))
        assert _blend(v0, v1 if two else None, wn_dev, off_dev, dims, o0, o1 if two else None) == N.WD_OK
        torch.cuda.synchronize()
        for name, buf, view in (("win0", b0, v0), ("win1", b1, v1), ("line0", o0buf, o0), ("line1", o1buf, o1)):
            G.assert_untouched(buf, view, name)
        got0, got1 = o0.reshape(lines, c, h, wl).cpu(), o1.reshape(lines, c, h, wl).cpu()
        G.assert_finite(got0, "line0")
        assert torch.equal(_bits(got0)[keep], _bits(want0)[keep]), ("line0", two)
        if two:
            G.assert_finite(got1, "line1")
            assert torch.equal(_bits(got1)[keep], _bits(want1)[keep])
        else:
            assert torch.equal(_bits(o1.cpu()), torch.full_like(_bits(o1.cpu()), G.NAN32))  # the absent line1 is not written
        outs.append(got0)
    assert _same_bits(outs[0], outs[1])  # line0 does not depend on whether a second prediction rides along
    assert torch.equal(v0.cpu().view(torch.int32), _bits(e0).reshape(-1)), "win0 was written"
    return want0, cover


@pytest.mark.parametrize("lines", [1, 3])
@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_kernels_bit_equal_to_the_specification(name, lines):
    c, h, w, wl, K, offs = LAYOUTS[name]
    off = np.array(offs[:lines], dtype=np.int64)
    g = torch.Generator().manual_seed(len(name) * 10 + lines)
    for kind in WEIGHTS:
        want, cover = _check_layout(c, h, w, wl, K, off, _weights(kind, lines, K, w, g), g)
        assert bool(cover.all()) == (name != "three-0-3-12")
        if name == "three-0-3-12":
            assert not cover[:, 11].any() and cover.sum() == lines * 19
    if name == "one":  # a single cover of weight 1: the value with its bits
        assert np.array_equal(W.normalise(off, np.ones((lines, 1, w), np.float32), wl, lines), np.ones((lines, 1, w), np.float32))


@pytest.mark.parametrize("lines", [1, 3])
def test_a_zero_weight_window_full_of_nan_does_not_reach_the_line(lines):
    g = torch.Generator().manual_seed(lines)
    # the middle window of three weighs nothing; the outer two cover the line
    c, h, w, wl, K, offs = LAYOUTS["three-deep"]
    off = np.array(offs[:lines], dtype=np.int64)
    wt = _weights("random", lines, K, w, g)
    wt[:, 1] = 0.0
    want, cover = _check_layout(c, h, w, wl, K, off, wt, g, nan_window=1)
    assert cover.all() and torch.isfinite(want).all()
    # two windows on the same columns, the first weighs nothing: the line IS the second, bit for bit
    off = np.zeros((lines, 2), dtype=np.int64)
    wt = np.ones((lines, 2, 8), dtype=np.float32)
    wt[:, 0] = 0.0
    _check_layout(4, 8, 8, 8, 2, off, wt, g, nan_window=0)


# ------------------------------------------------------------------------------------------------ 2. argument checks
def test_einval_launches_nothing():
    lines, K, c, h, w, wl = 2, 2, 4, 8, 8, 14
    g = torch.Generator().manual_seed(2)
    off = _i32(0, 6, 0, 6).reshape(lines, K)
    wn = torch.from_numpy(W.normalise(np.array([[0, 6]] * lines), np.ones((lines, K, w), np.float32), wl, lines)).to(DEV)
    line = torch.randn(lines * c * h * wl, generator=g).to(DEV)
    e0, e1 = (torch.randn(lines * K * c * h * w, generator=g).to(DEV) for _ in range(2))
    (wbuf, win), (l0buf, l0), (l1buf, l1) = (G.guarded_flat(k, torch.float32, device=DEV)
                                             for k in (lines * K * c * h * w, lines * c * h * wl, lines * c * h * wl))
    good = dict(lines=lines, K=K, c=c, h=h, w=w, wl=wl)
    shapes = [dict(K=0), dict(K=N.DEFINES["WD_WINDOW_MAX"] + 1), dict(K=-1), dict(w=0), dict(wl=w - 1), dict(lines=0), dict(c=0), dict(h=0)]

    def dims(**bad):
        d = dict(good, **bad)
        return tuple(d[k] for k in ("lines", "K", "c", "h", "w", "wl"))
    for bad in shapes:
        assert _gather(line, off, dims(**bad), win) == N.WD_EINVAL, bad
        assert _blend(e0, e1, wn, off, dims(**bad), l0, l1) == N.WD_EINVAL, bad
        assert _blend(e0, None, wn, off, dims(**bad), l0, None) == N.WD_EINVAL, bad
    for args in ((None, off, dims(), win), (line, None, dims(), win), (line, off, dims(), None)):
        assert _gather(*args) == N.WD_EINVAL
    for args in ((None, e1, wn, off, dims(), l0, l1), (e0, e1, None, off, dims(), l0, l1), (e0, e1, wn, None, dims(), l0, l1),
                 (e0, e1, wn, off, dims(), None, l1), (e0, e1, wn, off, dims(), l0, None), (e0, None, wn, off, dims(), l0, l1)):
        assert _blend(*args) == N.WD_EINVAL
    torch.cuda.synchronize()
    for name, buf, view in (("win", wbuf, win), ("line0", l0buf, l0), ("line1", l1buf, l1)):
        G.assert_untouched(buf, view, name)
        assert bool((view.cpu().view(torch.int32) == G.NAN32).all()), f"{name} was written"
    # ... and the calls themselves are good
    assert _gather(line, off, dims(), win) == N.WD_OK and _blend(e0, e1, wn, off, dims(), l0, l1) == N.WD_OK
    assert _blend(e0, None, wn, off, dims(K=1, wl=w), l0, None) == N.WD_OK
    torch.cuda.synchronize()
    for view in (win, l0, l1):
        G.assert_finite(view)


# ------------------------------------------------------------------------------------------------ the samplers
def _model(cls, cfg, seed, **args_kw):
    return fill_module_(cls(args=make_args(device=DEV, **args_kw), **cfg), seed).to(DEV).eval()


@pytest.fixture(scope="module")
def setup():
    args = make_args(device=DEV)
    m = _model(UNetModel, SMALL, 5)
    diff = Diffusion(noise_steps=T, img_size=HW, args=args)
    labels = torch.tensor([1, 7, 3, 9], dtype=torch.int64)
    lines = [["MOVE", "a", "Zebra"], ["quilt", "Moving", "on"], ["x", "Yak", "gnu"], ["Word", "by", "word"]]
    return m, diff, args, labels, lines


def _call(diff, which, m, n, x_text, labels, args, **kw):
    """One call of a sampler; the short schedules the tests share: 7 / 4 / 4 steps of T = 8."""
    if which == "ddpm":
        return diff.sampling(m, None, n, x_text, labels, args, **kw)
    if which == "ddim":
        return diff.sampling_ddim(m, None, n, x_text, labels, args, steps=4, **kw)
    return diff.sampling_dpmpp(m, None, n, x_text, labels, args, steps=4, spacing="time", **kw)


def _step_kernel(diff, which, x, eps, n, npix, k, tau, tabs, seed, offset, second=None, scale=0.0, eps_out=None, x0_prev=None,
                 noise=None):
    """The sampler's own update launch on (x, eps) at visited step k; returns (t_dev, k_dev) as ``wd_known_blend`` takes them."""
    lib = N.lib()
    if which == "ddpm":
        t_dev, k_dev = _i32(T - 1 - k), None
        N.check(lib.wd_ddpm_step(x.data_ptr(), eps.data_ptr(), n, npix, *(c.data_ptr() for c in tabs), t_dev.data_ptr(), _ptr(noise),
                                 seed, offset, _st()), "wd_ddpm_step")
    elif which == "ddim":
        t_dev, k_dev = _i32(tau[k]), _i32(k)
        N.check(lib.wd_ddim_step(x.data_ptr(), eps.data_ptr(), _ptr(second), scale, _ptr(eps_out), n, npix,
                                 *(c.data_ptr() for c in tabs), k_dev.data_ptr(), t_dev.data_ptr(), _ptr(noise), seed, offset, _st()),
                "wd_ddim_step")
    else:
        t_dev, k_dev = _i32(tau[k]), _i32(k)
        N.check(lib.wd_dpmpp_step(x.data_ptr(), eps.data_ptr(), _ptr(second), scale, _ptr(eps_out), x0_prev.data_ptr(), n, npix,
                                  *(c.data_ptr() for c in tabs), k_dev.data_ptr(), _st()), "wd_dpmpp_step")
    return t_dev, k_dev


# ------------------------------------------------------------------------------------------------ 3. K = 1 is the plain call
@pytest.mark.parametrize("which,eta", [("ddpm", None), ("ddim", 0.0), ("ddim", 0.5), ("dpmpp", None)])
def test_one_window_is_the_plain_call(setup, which, eta):
    m, diff, args, labels, lines = setup
    n, kw = 3, dict(seed=31, sample_offset=4, **({} if eta is None else dict(eta=eta)))
    words = [r[0] for r in lines[:n]]
    lw = diff.line_windows(n, 1)
    assert (lw.K, lw.w, lw.width) == (1, WM, WM) and bool((lw.wn == 1).all()) and not lw.offsets.any()
    rec0, rec1 = [], []
    plain = _call(diff, which, m, n, words, labels[:n], args, record=rec0, **kw)
    assert "windows" not in diff.last_stats
    line = _call(diff, which, m, n, [[v] for v in words], labels[:n], args, record=rec1, windows=lw, **kw)
    st = diff.last_stats
    assert (st["windows"], st["line_width"], st["model_batch"]) == (1, WM, n)
    assert len(rec0) == len(rec1) == st["steps"] and torch.isfinite(plain).all() and float(plain.std()) > 0.05
    for k, (a, b) in enumerate(zip(rec0 + [plain], rec1 + [line])):
        assert _same_bits(a, b), (which, k)
    # and through the captured graph
    again = _call(diff, which, m, n, [[v] for v in words], labels[:n], args, windows=lw, **kw)
    assert diff.last_stats["graph"] and _same_bits(again, plain)


# ------------------------------------------------------------------------------------------------ 4. disjoint windows: independent samples
def _split(x, K):
    """Line-shaped [n, C, h, K * w] -> the model batch [n * K, C, h, w] in model-batch order."""
    n = x.shape[0]
    return x.reshape(n, C, H, K, WM).permute(0, 3, 1, 2, 4).reshape(n * K, C, H, WM).contiguous()


@pytest.mark.parametrize("which", SAMPLERS)
def test_disjoint_windows_are_independent_samples(setup, which):
    m, diff, args, labels, lines = setup
    n, K = 2, 2
    lw = diff.line_windows(n, K, overlap=0)
    assert lw.width == 2 * WM and lw.offsets.tolist() == [[0, WM]] * n and bool((lw.wn == 1).all())
    g = torch.Generator().manual_seed(8)
    x_T = torch.randn(n, C, H, 2 * WM, generator=g)
    rows = [r[:K] for r in lines[:n]]
    kw, kw_plain = dict(x_T=x_T, seed=3), dict(x_T=_split(x_T, K), seed=3)
    if which == "ddpm":
        noise = [torch.randn(n, C, H, 2 * WM, generator=g) for _ in range(T - 2)]
        kw["noise"], kw_plain["noise"] = noise, [_split(z, K) for z in noise]
    got = _call(diff, which, m, n, rows, labels[:n], args, windows=lw, **kw)
    assert got.shape == (n, C, H, 2 * WM) and diff.last_stats["model_batch"] == n * K and diff.last_stats["graph"]
    want = _call(diff, which, m, n * K, [v for r in rows for v in r], labels[:n].repeat_interleave(K), args, **kw_plain)
    assert _same_bits(_split(got, K), want)
    assert not torch.equal(want[0], want[1]) and torch.isfinite(got).all()


# ------------------------------------------------------------------------------------------------ 5. every step through the C-ABI
@pytest.mark.parametrize("which,guided", [("ddpm", False), ("ddim", False), ("dpmpp", False), ("ddim", True)])
def test_every_step_of_a_masked_line_call_replays_through_the_c_abi(setup, which, guided):
    """record[k], the recorded window predictions, ``wd_window_blend``, the sampler's own step kernel on the line, then
    ``wd_known_blend``: record[k + 1] (and at the end the returned line), bit for bit."""
    m, diff, args, labels, lines = setup
    n, K, seed, offset, scale = 2, 3, 41, 5, 3.0
    lw = diff.line_windows(n, K, overlap=3, feather=2)
    wl = lw.width
    assert wl == 18 and lw.offsets.tolist() == [[0, 5, 10]] * n
    npix = C * H * wl
    g = torch.Generator().manual_seed(6)
    known = torch.randn(n, C, H, wl, generator=g) * 0.8
    soft = torch.zeros(H, wl)
    soft[:, :6] = 1.0
    soft[:, 6] = 0.5  # kept columns reach into the first overlap
    rec, preds = [], []
    extra = dict(guidance="writer_free", cfg_scale=scale) if guided else {}
    out = _call(diff, which, m, n, lines[:n], labels[:n], args, seed=seed, sample_offset=offset, known=known, known_mask=soft,
                record=rec, record_pred=preds, windows=lw, **extra)
    st = diff.last_stats
    assert (st["known"], st["graph"], st["windows"], st["line_width"], st["model_batch"]) == (True, False, K, wl, n * K)
    assert st["forwards_per_step"] == (2 if guided else 1)
    tau = st.get("timesteps")
    S = len(tau) if tau else T - 1
    assert len(rec) == len(preds) == S and out.shape == (n, C, H, wl)
    states = rec + [out]
    lib = N.lib()
    sa, sb = diff._noise_tables(DEV)
    x0 = known.reshape(n, -1).to(DEV)
    mask = soft.expand(n, C, H, wl).reshape(n, -1).contiguous().to(DEV)
    keps = None
    if st["known_noise"] == "fixed":
        keps = torch.empty(n, npix, device=DEV)
        N.check(lib.wd_randn(keps.data_ptr(), n, npix, seed, offset, N.STREAM_KNOWN, _st()), "wd_randn")
    tau_dev = None if tau is None else _i32(*tau)
    tabs = diff._step_tables(DEV) if which == "ddpm" else diff._ddim_tables(tau, 0.0, DEV) if which == "ddim" else diff._dpmpp_tables(tau, 2, DEV)
    x0_prev = torch.empty(n, npix, device=DEV)
    off_dev, wn_dev, dims = lw.offsets.to(DEV), lw.wn.to(DEV), (n, K, C, H, WM, wl)
    for k in range(S):
        x = states[k].clone()
        p = preds[k]
        assert len(p) == (5 if guided else 2) and p[0].shape == (n * K, C, H, WM) and p[-1].shape == (n, C, H, wl)
        e0, e1 = torch.empty(n, npix, device=DEV), (torch.empty(n, npix, device=DEV) if guided else None)
        assert _blend(p[0], p[1] if guided else None, wn_dev, off_dev, dims, e0, e1) == N.WD_OK
        torch.cuda.synchronize()
        assert _same_bits(e0.reshape(n, C, H, wl), p[2] if guided else p[1]), (which, k, "line prediction")
        eg = torch.empty(n, npix, device=DEV) if guided else None
        if guided:
            assert _same_bits(e1.reshape(n, C, H, wl), p[3])
        t_dev, k_dev = _step_kernel(diff, which, x, e0, n, npix, k, tau, tabs, seed, offset, second=e1, scale=scale if guided else 0.0,
                                    eps_out=eg, x0_prev=x0_prev)
        torch.cuda.synchronize()
        if guided:
            assert _same_bits(eg.reshape(n, C, H, wl), p[4]) and not torch.equal(p[4], p[2])
        assert not torch.equal(x, states[k + 1]), (k, "the known-region blend changed nothing")
        N.check(lib.wd_known_blend(x.data_ptr(), x0.data_ptr(), mask.data_ptr(), n, npix, sa.data_ptr(), sb.data_ptr(), _ptr(t_dev),
                                   _ptr(k_dev), _ptr(tau_dev), len(tau or ()), _ptr(keps), seed, offset, _st()), "wd_known_blend")
        torch.cuda.synchronize()
        assert _same_bits(x, states[k + 1]), (which, guided, k)
    assert torch.equal(out[..., :6].cpu(), known[..., :6]) and torch.isfinite(out).all()


def test_gather_of_the_state_is_the_models_input(setup):
    """``wd_window_gather`` of record[k], fed to a plain one-step call at batch n * K, gives the window predictions that a one-step
    windows call from x_T = record[k] records: what the model saw at that step is the gather of the line."""
    m, diff, args, labels, lines = setup
    n, K = 2, 3
    lw = diff.line_windows(n, K, overlap=3, feather=2)
    rec = []
    diff.sampling_ddim(m, None, n, lines[:n], labels[:n], args, steps=4, seed=9, record=rec, windows=lw)
    tau = diff.last_stats["timesteps"]
    words = [v for r in lines[:n] for v in r]
    for k, t in enumerate(tau):
        win = torch.full((n * K, C, H, WM), float("nan"), device=DEV)
        assert _gather(rec[k], lw.offsets.to(DEV), (n, K, C, H, WM, lw.width), win) == N.WD_OK
        torch.cuda.synchronize()
        assert _same_bits(win, torch.from_numpy(W.gather(rec[k].cpu().numpy(), lw.offsets.numpy(), WM)))
        p_line, p_plain = [], []
        diff.sampling_ddim(m, None, n, lines[:n], labels[:n], args, timesteps=[t], x_T=rec[k], record_pred=p_line, windows=lw)
        diff.sampling_ddim(m, None, n * K, words, labels[:n].repeat_interleave(K), args, timesteps=[t], x_T=win, record_pred=p_plain)
        assert len(p_line) == len(p_plain) == 1 and _same_bits(p_line[0][0], p_plain[0][0]), k


# ------------------------------------------------------------------------------------------------ 6. graph == eager
@pytest.mark.parametrize("which", SAMPLERS + ["skip"])
def test_graph_replay_equals_eager(setup, which):
    m, diff, args, labels, lines = setup
    n, K = 2, 3
    lw = diff.line_windows(n, K, overlap=2, feather=1)
    outs = []
    for use_graph in (True, False):
        if which == "skip":  # a DDPM call whose steps mostly reuse the previous line prediction, made the way ``sampling3`` makes it
            out = diff._sample("sampling3", m, None, n, lines[:n], labels[:n], args,
                               lambda: diff._ddpm(lambda i: i == T - 1 or i % 3 == 0, deterministic=True), bulk=True, cfg_scale=0,
                               seed=23, sample_offset=1, use_graph=use_graph, windows=lw)
            assert diff.last_stats["model_calls"] == 3 and diff.last_stats["steps"] == T - 1
        else:
            out = _call(diff, which, m, n, lines[:n], labels[:n], args, seed=23, sample_offset=1, use_graph=use_graph, windows=lw)
        assert diff.last_stats["graph"] == use_graph and diff.last_stats["windows"] == K
        outs.append(out)
    assert _same_bits(outs[0], outs[1]) and torch.isfinite(outs[0]).all() and outs[0].shape == (n, C, H, lw.width)
    m.eval()


# ------------------------------------------------------------------------------------------------ 7. one float64 trajectory
def test_line_ddim_trajectory_matches_float64_oracle():
    """DDIM, eta = 0, 4 visited steps, 2 lines of 2 different words, overlap 4, feather 3: every state against the CPU oracle UNet
    per window, with the blend and the update (``tests/_ddim_ref.py``) in float64."""
    S, n, K, seed = 4, 2, 2, 9
    args = make_args(device=DEV)
    m = _model(UNetModel, SMALL, seed)
    diff = Diffusion(noise_steps=T, img_size=HW, args=args)
    tau = diff.ddim_timesteps(S)
    lw = diff.line_windows(n, K, overlap=4, feather=3)
    wl = lw.width
    assert tau == [7, 5, 3, 1] and wl == 12
    g = torch.Generator().manual_seed(3)
    x_T = torch.randn(n, C, H, wl, generator=g)
    labels = torch.tensor([1, 7], dtype=torch.int64)
    rows = [["Moving", "on"]] * n
    rec = []
    out = diff.sampling_ddim(m, None, n, rows[0], labels, args, steps=S, eta=0.0, x_T=x_T, record=rec, windows=lw)
    assert diff.last_stats["model_calls"] == S and diff.last_stats["model_batch"] == n * K
    sd = {k: torch.from_numpy(synthetic_tensor(k, s, seed)).double() for k, s in U.state_dict_shapes(SMALL, "base")}
    orc = U.UNetOracle(SMALL, sd, "base", False)
    ctx = torch.tensor([D.label_padding(v) for r in rows for v in r], dtype=torch.int64)
    y = labels.repeat_interleave(K)
    c = R.tables(T, tau, 0.0)
    off = lw.offsets.numpy()
    x, ref = x_T.double(), []
    with torch.no_grad():
        for k, t in enumerate(tau):
            ref.append(x.clone())
            win = torch.from_numpy(W.gather(x.numpy(), off, WM))
            e = orc(win, torch.full((n * K,), t, dtype=torch.int64), ctx, y, None).double()
            eps = torch.from_numpy(W.blend(e.numpy(), lw.wn.numpy(), off, wl, dtype=np.float64))
            x = R.step(c, k, x, eps)
    xs = torch.stack([r.cpu() for r in rec] + [out.cpu()])
    ref_xs = torch.stack(ref + [x])
    assert xs.shape == ref_xs.shape == (S + 1, n, C, H, wl)
    errs = [max_rel(xs[k], ref_xs[k]) for k in range(S + 1)]
    print(f"line ddim trajectory: max_rel per state {['%.2e' % e for e in errs]}")
    assert max(errs) < 1e-4


# ------------------------------------------------------------------------------------------------ 8. keyed by the global line
def test_lines_are_keyed_by_the_global_line(setup):
    m, diff, args, labels, lines = setup
    K, seed = 2, 29
    wl = diff.line_windows(1, K, overlap=2).width
    npix = C * H * wl
    tabs = diff._step_tables(DEV)
    runs = {}
    for lo, n in ((0, 4), (2, 2)):
        rec, preds = [], []
        diff.sampling(m, None, n, [r[:K] for r in lines[lo:lo + n]], labels[lo:lo + n], args, seed=seed, sample_offset=lo, record=rec,
                      record_pred=preds, windows=diff.line_windows(n, K, overlap=2))
        runs[lo] = (rec, preds)
    whole, part = runs[0], runs[2]
    assert _same_bits(whole[0][0][2:], part[0][0])  # x_T of lines 2, 3
    assert not torch.equal(whole[0][0][:2], part[0][0])
    # the first step's draw, isolated: the step kernel on rows 2, 3 alone with sample_offset = 2 and the recorded line prediction
    for (rec, preds), rows in ((whole, slice(2, 4)), (part, slice(0, 2))):
        x = rec[0][rows].clone()
        eps = preds[0][1][rows].contiguous()
        _step_kernel(diff, "ddpm", x, eps, 2, npix, 0, None, tabs, seed, 2)
        torch.cuda.synchronize()
        assert _same_bits(x, rec[1][rows])
        zero = x.clone()  # the same update without the noise term differs: the step did draw
        zero.copy_(rec[0][rows])
        _step_kernel(diff, "ddpm", zero, eps, 2, npix, 0, None, tabs, seed, 2, noise=torch.zeros(2, npix, device=DEV))
        torch.cuda.synchronize()
        assert not torch.equal(zero, x)
    # the draw itself: both calls' noise terms from the same (x, eps) are the same bits
    x_a, x_b = whole[0][0][2:].clone(), part[0][0].clone()
    eps = whole[1][0][1][2:].contiguous()
    _step_kernel(diff, "ddpm", x_a, eps, 2, npix, 0, None, tabs, seed, 2)
    _step_kernel(diff, "ddpm", x_b, eps, 2, npix, 0, None, tabs, seed, 2)
    torch.cuda.synchronize()
    assert _same_bits(x_a, x_b) and _same_bits(x_a, whole[0][1][2:])


# ------------------------------------------------------------------------------------------------ 9. PHOSC
def test_phosc_labels_in_either_shape_and_disjoint_windows():
    n, K = 2, 2
    args = make_args(device=DEV, phosc=1)
    m = _model(UNetModelPhosc, SMALL, 6, phosc=1)
    diff = Diffusion(noise_steps=T, img_size=HW, args=args)
    g = torch.Generator().manual_seed(4)
    ph = torch.randint(0, 2, (n, K, 37), generator=g)
    labels = torch.tensor([2, 8], dtype=torch.int64)
    rows = [["Moving", "on"], ["a", "Zebra"]]
    lw = diff.line_windows(n, K, overlap=3, feather=1)
    a = diff.sampling_ddim(m, None, n, rows, labels, args, steps=4, seed=5, phoscLabels=ph, windows=lw)
    b = diff.sampling_ddim(m, None, n, rows, labels, args, steps=4, seed=5, phoscLabels=ph.reshape(n * K, 37), windows=lw)
    assert _same_bits(a, b) and torch.isfinite(a).all() and a.shape == (n, C, H, lw.width)
    other = diff.sampling_ddim(m, None, n, rows, labels, args, steps=4, seed=5, phoscLabels=1 - ph, windows=lw)
    assert not torch.equal(a, other)  # the labels reach the model
    # disjoint windows: the plain call at batch n * K on the split x_T
    lw0 = diff.line_windows(n, K, overlap=0)
    x_T = torch.randn(n, C, H, K * WM, generator=g)
    got = diff.sampling_ddim(m, None, n, rows, labels, args, steps=4, x_T=x_T, phoscLabels=ph, windows=lw0)
    want = diff.sampling_ddim(m, None, n * K, [v for r in rows for v in r], labels.repeat_interleave(K), args, steps=4, x_T=_split(x_T, K),
                              phoscLabels=ph.reshape(n * K, 37))
    assert _same_bits(_split(got, K), want)


# ------------------------------------------------------------------------------------------------ 10. model state and refusals
def test_model_state_and_refusals(setup):
    import random
    m, diff, args, labels, lines = setup
    n, K = 2, 3
    lw = diff.line_windows(n, K, overlap=2)
    m.eval()
    out = diff.sampling_dpmpp(m, None, n, lines[:n], labels[:n], args, steps=3, windows=lw)
    assert m.training and out.shape == (n, C, H, lw.width)  # eval mode for the loop, TRAIN mode afterwards, as without windows
    mi = _model(UNetModel, SMALL, 5, interpolation=True)
    iargs = make_args(device=DEV, interpolation=True)
    refused = [(m, args, dict(attention=True)), (m, args, dict(attention=(7, 1))), (m, args, dict(style_pairs=(1, 2), mix_rate=0.5)),
               (mi, iargs, dict(mix_rate=0.5))]
    for model, a, kw in refused:
        for call, extra in ((diff.sampling, {}), (diff.sampling_ddim, dict(steps=3)), (diff.sampling_dpmpp, dict(steps=3))):
            model.train()
            random.seed(3)
            torch.manual_seed(3)
            rs, ts = random.getstate(), torch.random.get_rng_state()
            with pytest.raises(NotImplementedError):
                call(model, None, n, lines[:n], labels[:n], a, windows=lw, **extra, **kw)
            assert model.training and random.getstate() == rs and torch.equal(torch.random.get_rng_state(), ts), sorted(kw)
    m.eval()


# ------------------------------------------------------------------------------------------------ 11. driver
def test_driver_lines(tmp_path, monkeypatch):
    from worddiffusion_amd import driver
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    text = tmp_path / "lines.txt"
    text.write_text("w1\tMoving on\nw2\ta Zebra\nw1\tWord by word\n")
    args = make_args(device=DEV)
    kw = dict(image_size=(64, 256), in_channels=4, model_channels=64, out_channels=4, num_res_blocks=1, attention_resolutions=(1, 1),
              channel_mult=(1, 1), num_heads=2, num_classes=339, context_dim=64, vocab_size=53, max_seq_len=10)
    m = fill_module_(UNetModel(args=args, **kw), 17)
    os.makedirs(tmp_path / "run" / "models")
    torch.save(m.state_dict(), tmp_path / "run" / "models" / "ema_ckpt.pt")
    out = tmp_path / "out"
    calls = []
    real = Diffusion.sampling_ddim

    def spy(self, model, vae, n, x_text, labels, a, **kws):
        res = real(self, model, vae, n, x_text, labels, a, **kws)
        calls.append((n, self.last_stats["windows"], self.last_stats["model_batch"], self.last_stats["line_width"]))
        return res
    monkeypatch.setattr(Diffusion, "sampling_ddim", spy)
    driver.main(["--lines", str(text), "--models_path", str(tmp_path / "run"), "--save_path", str(out), "--writer_dict",
                 str(tmp_path / "writers.json"), "--batch_size", "4", "--emb_dim", "64", "--num_heads", "2", "--noise_steps", "11",
                 "--seed", "5", "--sampler", "ddim", "--ddim_steps", "3", "--line_overlap", "4", "--line_feather", "2"])
    assert sorted(os.listdir(out / "images")) == ["line_0.npy", "line_1.npy", "line_2.npy"]
    widths = [np.load(out / "images" / f"line_{i}.npy").shape for i in range(3)]
    assert widths == [(4, 8, 60), (4, 8, 60), (4, 8, 88)]
    assert sorted(calls) == [(1, 3, 3, 88), (2, 2, 4, 60)]  # the 2-word group is one call of model batch 4
    for i in range(3):
        assert np.isfinite(np.load(out / "images" / f"line_{i}.npy")).all()
