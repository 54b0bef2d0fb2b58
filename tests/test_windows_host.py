"""Line sampling (``windows=``), the part that needs no GPU: ``window_profile``, ``Diffusion.line_windows`` against the numpy
specification (``tests/_window_ref.py``), the identities of the specification itself, the exported symbols and the argument handling
of the three samplers.

Bounds: the normalised weights of a column are K fp32 roundings of float64 quotients that sum to 1, each within 2^-25 of its
quotient (every quotient is <= 1), so their float64 sum is within K * 2^-25 < K * 2^-24 of 1."""
import numpy as np
import pytest
import torch

from tests import _window_ref as W
from tests._common import SMALL, make_args
from worddiffusion_amd import Diffusion, LineWindows, UNetModel, window_profile
from worddiffusion_amd import _native as N

HW = (64, 64)
C, H, WM = 4, 8, 8
NAN = np.array([0x7FFBADAD], dtype=np.uint32).view(np.float32)[0]


def _diff(hw=HW):
    return Diffusion(noise_steps=8, img_size=hw)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ window_profile
@pytest.mark.parametrize("w,feather,want", [
    (8, 0, [1] * 8),
    (8, 3, [0.25, 0.5, 0.75, 1, 1, 0.75, 0.5, 0.25]),
    (26, 5, [k / 6 for k in range(1, 6)] + [1] * 16 + [k / 6 for k in range(5, 0, -1)])])
def test_window_profile(w, feather, want):
    p = window_profile(w, feather)
    assert p.dtype == torch.float32 and tuple(p.shape) == (w,)
    assert np.array_equal(p.numpy(), np.array(want, dtype=np.float64).astype(np.float32))
    assert np.array_equal(p.numpy(), W.profile(w, feather)) and torch.equal(p, p.flip(0))
    if feather == 0:
        assert torch.equal(window_profile(w), p)
    with pytest.raises(ValueError):
        window_profile(0)
    with pytest.raises(ValueError):
        window_profile(8, -1)


# ------------------------------------------------------------------------------------------------ line_windows
def test_line_windows_defaults():
    d = _diff()
    lw = d.line_windows(3, 4, overlap=2)
    assert isinstance(lw, LineWindows) and (lw.K, lw.w, lw.width) == (4, WM, 4 * WM - 3 * 2)
    assert lw.offsets.dtype == torch.int32 and lw.offsets.tolist() == [[0, 6, 12, 18]] * 3
    assert lw.wn.dtype == torch.float32 and tuple(lw.wn.shape) == (3, 4, WM)
    assert np.array_equal(lw.wn.numpy(), W.normalise(lw.offsets.numpy(), np.ones(WM, np.float32), lw.width, 3))
    assert lw.wn[0, 0].tolist() == [1, 1, 1, 1, 1, 1, 0.5, 0.5] and lw.wn[0, 1].tolist() == [0.5, 0.5, 1, 1, 1, 1, 0.5, 0.5]
    with pytest.raises(AttributeError):
        lw.width = 3  # immutable
    one = d.line_windows(2, 1)
    assert (one.K, one.width) == (1, WM) and bool((one.wn == 1).all()) and not one.offsets.any()
    # the model's width comes from img_size
    assert _diff((64, 256)).line_windows(1, 3, overlap=2).width == 3 * 32 - 4
    # feather is the default weight; an explicit weight of the same values is the same table
    f = d.line_windows(2, 3, overlap=3, feather=2)
    assert torch.equal(f.wn, d.line_windows(2, 3, overlap=3, weight=window_profile(WM, 2)).wn)
    assert torch.equal(f.wn, d.line_windows(2, 3, overlap=3, weight=window_profile(WM, 2).expand(3, WM)).wn)
    assert torch.equal(f.wn, d.line_windows(2, 3, overlap=3, weight=window_profile(WM, 2).expand(2, 3, WM)).wn)
    # explicit offsets, [K] and [n, K], with a width
    a = d.line_windows(2, 3, offsets=[0, 4, 12], width=20)
    b = d.line_windows(2, 3, offsets=torch.tensor([[0, 4, 12], [0, 8, 12]]), width=20)
    assert a.offsets.tolist() == [[0, 4, 12]] * 2 and b.offsets.tolist() == [[0, 4, 12], [0, 8, 12]] and a.width == b.width == 20
    assert torch.equal(a.wn[0], b.wn[0]) and not torch.equal(a.wn[1], b.wn[1])


def test_line_windows_errors():
    d = _diff()
    for kw in (dict(offsets=[0, 13], width=20), dict(offsets=[-1, 6], width=14), dict(offsets=[[0, 6], [0, 7]], width=14),
               dict(offsets=[0, 6]),                           # the default width (16) leaves the offsets valid but ...
               dict(offsets=[0.0, 6.0], width=14), dict(offsets=[0, 6, 12], width=20),
               dict(weight=-window_profile(WM)), dict(weight=torch.tensor([1.0] * 7 + [-1e-9])), dict(weight=torch.ones(7)),
               dict(weight=torch.full((WM,), float("nan"))), dict(overlap=WM), dict(overlap=-1), dict(width=WM - 1)):
        if kw == dict(offsets=[0, 6]):  # ... 0, 6 of width 16 leaves columns 14, 15 uncovered
            with pytest.raises(ValueError, match=r"line 0: column 14"):
                d.line_windows(2, 2, **kw)
            continue
        with pytest.raises(ValueError):
            d.line_windows(2, 2, **kw)
    with pytest.raises(ValueError, match="WD_WINDOW_MAX"):
        d.line_windows(1, N.DEFINES["WD_WINDOW_MAX"] + 1)
    assert d.line_windows(1, N.DEFINES["WD_WINDOW_MAX"], overlap=4).K == 32
    for n, K in ((0, 2), (2, 0)):
        with pytest.raises(ValueError):
            d.line_windows(n, K)
    # an uncovered column: the message names the line and the column
    with pytest.raises(ValueError, match=r"line 1: column 0\b"):
        d.line_windows(2, 2, offsets=[[0, 8], [1, 8]], width=16)
    w0 = window_profile(WM).clone()
    w0[0] = 0.0  # the first column of every window weighs nothing: column 0 of the line has no cover
    with pytest.raises(ValueError, match=r"line 0: column 0\b"):
        d.line_windows(2, 2, overlap=2, weight=w0)
    zero = torch.ones(2, 2, WM)
    zero[1, 1] = 0.0  # a whole window without weight is fine where the others cover ...
    assert d.line_windows(2, 2, offsets=[0, 0], width=WM, weight=zero).wn[1].tolist() == [[1.0] * WM, [0.0] * WM]
    with pytest.raises(ValueError, match=r"line 1: column 8\b"):  # ... and an error where they do not
        d.line_windows(2, 2, overlap=0, weight=zero)


def _random_layout(rng, K, w):
    """Offsets that cover a line of random width, and positive random weights on a random scale (1e-3 .. 1e3)."""
    steps = rng.integers(1, w + 1, size=K - 1)
    off = np.concatenate([[0], np.cumsum(steps)]).astype(np.int64)
    width = int(off[-1]) + w
    wt = rng.uniform(0.05, 1.0, size=(K, w)).astype(np.float32) * np.float32(10.0) ** rng.integers(-3, 4)
    return off, width, wt


def test_partition_of_unity_over_random_layouts():
    d = _diff()
    rng = np.random.default_rng(11)
    worst_ref, singles = 0.0, 0
    for _ in range(2000):
        K = int(rng.integers(1, 7))
        off, width, wt = _random_layout(rng, K, WM)
        lw = d.line_windows(1, K, offsets=off.tolist(), width=width, weight=torch.from_numpy(wt))
        ref = W.normalise(off[None], wt, width, 1)
        assert np.array_equal(lw.wn.numpy(), ref)  # the product's table IS the specification's
        tot = np.zeros(width)
        cnt = np.zeros(width, dtype=np.int64)
        for k in range(K):
            tot[off[k]:off[k] + WM] += ref[0, k].astype(np.float64)
            cnt[off[k]:off[k] + WM] += 1
        assert (cnt >= 1).all()
        err = np.abs(tot - 1.0)
        assert (err <= cnt * 2.0 ** -24).all() and err.max() <= K * 2.0 ** -24
        worst_ref = max(worst_ref, float(err.max()))
        single = cnt == 1  # a single cover: exactly 1.0
        singles += int(single.sum())
        for k in range(K):
            cols = np.arange(off[k], off[k] + WM)
            assert (ref[0, k][single[cols]] == 1.0).all()
    print(f"partition of unity: worst |sum - 1| = {worst_ref / 2.0 ** -24:.3f} * 2^-24 over 2000 layouts; {singles} single covers")
    assert worst_ref < 2.0 ** -24 and singles > 1000


# ------------------------------------------------------------------------------------------------ the specification's identities
def test_one_window_blend_returns_the_bits():
    g = np.random.default_rng(2)
    e = g.standard_normal((2, C, H, WM)).astype(np.float32)
    e[0, 0, 0, 0], e[1, 1, 2, 3], e[0, 2, 1, 5] = -0.0, NAN, np.float32("inf")
    wn = np.ones((2, 1, WM), dtype=np.float32)
    got = W.blend(e, wn, np.zeros((2, 1), dtype=np.int64), WM)
    assert np.array_equal(_bits(got), _bits(e))
    assert np.signbit(got[0, 0, 0, 0]) and _bits(got)[1, 1, 2, 3] == 0x7FFBADAD


def test_a_zero_weight_window_does_not_reach_the_line():
    g = np.random.default_rng(3)
    off = np.array([[0, 3, 6]])
    wt = np.ones((1, 3, WM), dtype=np.float32)
    wt[0, 1] = 0.0
    wn = W.normalise(off, wt, 14, 1)
    assert (wn[0, 1] == 0).all() and (W.coverage(off, wt, 14, 1) > 0).all()
    e = g.standard_normal((3, C, H, WM)).astype(np.float32)
    e[1] = NAN
    got = W.blend(e, wn, off, 14)
    assert np.isfinite(got).all()
    e2 = e.copy()
    e2[1] = 7.0
    assert np.array_equal(_bits(got), _bits(W.blend(e2, wn, off, 14)))
    # ... while a weighted one does
    assert np.isnan(W.blend(e, W.normalise(off, np.ones((1, 3, WM), np.float32), 14, 1), off, 14)).any()


def test_gather_then_flat_blend_returns_the_line():
    g = np.random.default_rng(4)
    deepest = 0
    for off, width in (([[0, 6]], 14), ([[0, 3, 6]], 14), ([[0, 6, 12], [0, 4, 12]], 20), ([[0, 0, 0, 0]], 8)):
        off = np.array(off)
        n, K = off.shape
        line = g.standard_normal((n, C, H, width)).astype(np.float32)
        line[0, 0, 0, 0] = -0.0
        win = W.gather(line, off, WM)
        assert win.shape == (n * K, C, H, WM)
        for s in range(n):
            for k in range(K):
                assert np.array_equal(_bits(win[s * K + k]), _bits(line[s, :, :, off[s, k]:off[s, k] + WM]))
        wt = np.ones((n, K, WM), dtype=np.float32)
        back = W.blend(win, W.normalise(off, wt, width, n), off, width)
        cnt = W.coverage(off, wt, width, n).astype(np.int64)  # flat weights: the sum counts the covering windows
        assert (cnt >= 1).all()
        single = np.broadcast_to((cnt == 1)[:, None, None, :], line.shape)
        assert np.array_equal(_bits(back)[single], _bits(line)[single])
        # equal values under several covers: within 1 ulp per extra window (each 1/c and each sum rounds once)
        ulp = np.spacing(np.abs(line))
        extra = np.broadcast_to((cnt - 1)[:, None, None, :], line.shape)
        assert (np.abs(back.astype(np.float64) - line) <= extra * ulp).all()
        deepest = max(deepest, int(cnt.max()))
    assert deepest == 4  # columns under two, three and four windows were all seen


# ------------------------------------------------------------------------------------------------ the library
def test_symbols_are_exported():
    lib = N.lib()
    assert N.DEFINES["WD_WINDOW_MAX"] == 32
    for name in ("wd_window_gather", "wd_window_blend"):
        assert name in N.header_symbols() and getattr(lib, name) is not None


# ------------------------------------------------------------------------------------------------ the samplers' argument handling
CALLS = [("sampling", {}), ("sampling_ddim", dict(steps=3)), ("sampling_dpmpp", dict(steps=3))]


@pytest.mark.parametrize("name,extra", CALLS)
def test_sampler_arguments_with_windows(name, extra):
    import random
    d = _diff()
    call = getattr(d, name)
    args = make_args()  # device "cpu": a call that passes its argument handling ends at "runs on an MI355X only"
    m = UNetModel(args=args, **SMALL)
    n, K = 2, 3
    lw = d.line_windows(n, K, overlap=2)
    labels = torch.tensor([1, 2], dtype=torch.int64)
    rows = [["a", "bc", "d"], ["e", "f", "gh"]]
    for good in (rows, rows[0], [tuple(r) for r in rows]):
        with pytest.raises(N.NativeError, match="MI355X"):
            call(m, None, n, good, labels, args, windows=lw, **extra)
    # x_text nesting
    for bad in ("word", ["a", "b"], [["a", "b", "c"]], [["a", "b"], ["c", "d"]], [["a", "b", "c"], "def"], [["a", "b", 3], ["d", "e", "f"]],
                ["a", "b", "c", "d", "e", "f"]):
        with pytest.raises(ValueError, match="x_text"):
            call(m, None, n, bad, labels, args, windows=lw, **extra)
    # labels: one writer per line
    with pytest.raises(ValueError, match="labels"):
        call(m, None, n, rows, labels.repeat_interleave(K), args, windows=lw, **extra)
    # PHOSC labels: [n, K, L] or [n * K, L]
    pargs = make_args(phosc=1)
    for ok in (torch.zeros(n, K, 5, dtype=torch.int64), torch.zeros(n * K, 5, dtype=torch.int64)):
        with pytest.raises(N.NativeError, match="MI355X"):
            call(m, None, n, rows, labels, pargs, phoscLabels=ok, windows=lw, **extra)
    with pytest.raises(ValueError, match="phoscLabels"):
        call(m, None, n, rows, labels, pargs, phoscLabels=torch.zeros(n, 5, dtype=torch.int64), windows=lw, **extra)
    # known: line-shaped
    mask = torch.ones(H, lw.width)
    with pytest.raises(N.NativeError, match="MI355X"):
        call(m, None, n, rows, labels, args, windows=lw, known=torch.zeros(n, C, H, lw.width), known_mask=mask, **extra)
    for known, km in ((torch.zeros(n, C, H, WM), mask), (torch.zeros(n * K, C, H, WM), mask), (torch.zeros(n, C, H, lw.width), torch.ones(H, WM))):
        with pytest.raises(ValueError, match="known"):
            call(m, None, n, rows, labels, args, windows=lw, known=known, known_mask=km, **extra)
    # a layout of another call
    with pytest.raises(ValueError, match="windows"):
        call(m, None, 3, rows + [rows[0]], torch.tensor([1, 2, 3]), args, windows=lw, **extra)
    with pytest.raises(ValueError, match="windows"):
        call(m, None, n, rows, labels, args, windows=_diff((64, 256)).line_windows(n, K), **extra)
    with pytest.raises(TypeError):
        call(m, None, n, rows, labels, args, windows=(lw.offsets, lw.wn), **extra)
    # refused combinations: before anything is drawn
    mi = UNetModel(args=make_args(interpolation=True), **SMALL)
    for model, kw in ((m, dict(attention=True)), (m, dict(attention=(5, 1))), (m, dict(style_pairs=(1, 2), mix_rate=0.5)),
                      (mi, dict(mix_rate=0.5))):
        model.train()
        random.seed(5)
        torch.manual_seed(5)
        rs, ts = random.getstate(), torch.random.get_rng_state()
        with pytest.raises(NotImplementedError):
            call(model, None, n, rows, labels, args, windows=lw, **kw, **extra)
        assert model.training and random.getstate() == rs and torch.equal(torch.random.get_rng_state(), ts)
    # attention=False / None and a mix_rate the model ignores are the plain line call
    with pytest.raises(N.NativeError, match="MI355X"):
        call(m, None, n, rows, labels, args, windows=lw, attention=False, mix_rate=0.5, **extra)


def test_sampling3_refuses_windows():
    d = _diff()
    args = make_args()
    m = UNetModel(args=args, **SMALL)
    m.train()
    with pytest.raises(NotImplementedError, match="sampling3"):
        d.sampling3(0, None, ["a"] * 2, None, m, m, None, 0, 1, 2, ["a"] * 2, torch.tensor([1, 2]), args, windows=d.line_windows(2, 1))
    assert m.training  # refused before the model was touched


def test_driver_lines_flags(tmp_path):
    from worddiffusion_amd import driver
    ap, a = driver.parse_args(["--lines", "l.txt", "--save_path", "out"])
    assert (a.lines, a.line_overlap, a.line_feather, a.gt_train) == ("l.txt", 2, 0, None)
    ap, a = driver.parse_args(["--lines", "l.txt", "--save_path", "out", "--line_overlap", "5", "--line_feather", "3", "--sampler", "dpmpp"])
    assert (a.line_overlap, a.line_feather, a.sampler) == (5, 3, "dpmpp")
    for bad in (["--save_path", "out"], ["--lines", "l", "--save_path", "o", "--gt_train", "g"], ["--lines", "l", "--save_path", "o", "--skip_steps", "1"],
                ["--lines", "l", "--save_path", "o", "--style_pair", "1", "2"], ["--lines", "l", "--save_path", "o", "--mix_rate", "0.5"],
                ["--lines", "l", "--save_path", "o", "--attn_maps", "m"], ["--lines", "l", "--save_path", "o", "--line_overlap", "32"],
                ["--lines", "l", "--save_path", "o", "--line_feather", "-1"]):
        with pytest.raises(SystemExit):
            driver.parse_args(bad)
    f = tmp_path / "lines.txt"
    f.write_text("w1\tMoving on\n\nw2\t a  Zebra \nw1\tWord by word\n")
    assert driver.read_lines(str(f)) == [("w1", ("Moving", "on")), ("w2", ("a", "Zebra")), ("w1", ("Word", "by", "word"))]
    for text in ("w1 Moving on\n", "w1\t\n", "\tMoving\n"):
        f.write_text(text)
        with pytest.raises(ValueError, match="row 1"):
            driver.read_lines(str(f))
