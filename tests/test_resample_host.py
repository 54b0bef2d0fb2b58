"""Resampling jumps (``resample=``, ``jump=``), the part that needs no GPU: the walk and its per-entry tables against the
specification (``tests/_resample_ref.py``), the identities of the specification itself, the tag families of the noise stream,
the exported symbols and the argument handling of the samplers.

Bounds: a table entry is one fp32 rounding of a float64 value, so library and specification agree in every bit unless their
float64 values differ in the last place - they are compared to 2 ulp of fp32 relative (2^-22), and bit for bit where both
sides are the library's.  g1^2 + g2^2: each factor is within 2^-24 relative of its float64 value, whose squares sum to 1, so
the float64 sum of the fp32 squares is within 2 * 2^-24 * (g1^2 + g2^2) + O(2^-48) < 2^-22 of 1."""
import random

import numpy as np
import pytest
import torch

from tests import _resample_ref as R
from tests._common import SMALL, make_args
from worddiffusion_amd import Diffusion, UNetModel
from worddiffusion_amd import _native as N
from worddiffusion_amd import diffusion as DM

T = 60
CASES = [(4, 2, 2), (5, 2, 3), (4, 1, 2), (4, 4, 3), (4, 5, 2), (7, 3, 2), (50, 10, 10)]
ULP2 = 2.0 ** -22


def _diff(T=T):
    return Diffusion(noise_steps=T, img_size=(32, 64))


def _tau(d, S):
    return d.ddim_timesteps(S)


# ------------------------------------------------------------------------------------------------ the walk
@pytest.mark.parametrize("S,j,r", CASES)
def test_walk_counts_and_continuity(S, j, r):
    d = _diff()
    tau = _tau(d, S)
    ref = R.walk(tau, j, r)
    downs, ups = R.counts(S, j, r)
    assert sum(e[0] == "down" for e in ref) == downs == S + (r - 1) * ((S - 1) // j) * j
    assert sum(e[0] == "up" for e in ref) == ups == (r - 1) * ((S - 1) // j)
    # each entry starts at the level the previous one reached; the first starts at tau[0], the last ends at 0
    assert ref[0][1] == tau[0] and ref[-1][2] == 0
    assert all(a[2] == b[1] for a, b in zip(ref, ref[1:]))
    # a down entry goes down the schedule by one visited step, an up entry up by j of them
    for kind, frm, to, m in ref:
        if kind == "down":
            assert frm == tau[m] and to == (tau[m + 1] if m + 1 < S else 0) and to < frm
        else:
            assert to > frm and tau.index(frm) - tau.index(to) == j
    # every plain step is taken r times, except those of the last stretch, which no jump follows
    taken = [sum(e[3] == m for e in ref) for m in range(S)]
    last = ((S - 1) // j) * j
    assert taken == [r] * last + [1] * (S - last)
    # the library's walk is that walk
    w = d.resample_walk(tau, j, r)
    assert (w.tau, w.to, w.up) == ([e[1] for e in ref], [e[2] for e in ref], [e[0] == "up" for e in ref])
    assert (w.resample, w.jump) == (r, j) and w.down == [k for k, e in enumerate(ref) if e[0] == "down"]


def test_the_example_of_the_specification():
    ref = R.walk([7, 5, 3, 1], 2, 2)
    assert [(e[0], e[1], e[2]) for e in ref] == [("down", 7, 5), ("down", 5, 3), ("up", 3, 7), ("down", 7, 5), ("down", 5, 3),
                                                 ("down", 3, 1), ("down", 1, 0)]


@pytest.mark.parametrize("S,j,r", [(4, 2, 1), (7, 3, 1), (4, 4, 3), (4, 5, 2), (1, 1, 5)])
def test_r1_or_a_long_jump_is_the_plain_schedule(S, j, r):
    d = _diff()
    tau = _tau(d, S)
    ref = R.walk(tau, j, r)
    assert [e[1] for e in ref] == tau and all(e[0] == "down" for e in ref) and [e[3] for e in ref] == list(range(S))
    w = d.resample_walk(tau, j, r)
    assert w.tau == tau and not any(w.up) and not w.g1.any() and not w.g2.any()
    # ... and its tables are the plain call's, bit for bit
    for eta in (0.0, 0.7):
        plain, walked = d._ddim(tau, eta), d._ddim(tau, eta, w)
        assert [s[:2] for s in walked.steps] == [s[:2] for s in plain.steps] and walked.tau == plain.tau
    for a, b in zip(d._ddim_tables(tau, 0.7, "cpu"), d._ddim_tables(tau, 0.7, "cpu", to=tau[1:] + [0])):
        assert torch.equal(a, b)
    for a, b in zip(d._dpmpp_tables(tau, 2, "cpu"), d._dpmpp_tables(tau, 2, "cpu", to=tau[1:] + [0], restart=[])):
        assert torch.equal(a, b)


def test_resample_1_builds_the_plain_sampler():
    """``resample=1`` (or absent) settles to no walk at all: the ``_Sampler`` the call had before the argument existed."""
    d = _diff()
    assert d._resample_setup(None, [7, 5, 3, 1], 1, 10, None) is None
    assert d._resample_setup(None, [7, 5, 3, 1], 1, 1, None, attention=True, style_pairs=(1, 2), mix_rate=0.5) is None
    assert d._ddim([7, 5, 3, 1], 0.5, None).walk is None and d._dpmpp([7, 5, 3, 1], 2, None, None).walk is None
    assert d._ddpm(walk=None).walk is None and d._ddpm().steps == d._ddpm(walk=None).steps and d._ddpm().tau is None


def test_walk_limit_names_itself():
    d = _diff(1000)
    d.resample_walk(range(999, 0, -1), 10, 10)  # RePaint's own setting on the full schedule fits
    with pytest.raises(ValueError, match=str(DM.WALK_MAX)):
        d.resample_walk(range(999, 0, -1), 1, 20)


# ------------------------------------------------------------------------------------------------ the tables
@pytest.mark.parametrize("S,j,r", CASES)
def test_jump_tables(S, j, r):
    d = _diff()
    tau = _tau(d, S)
    ref = R.walk(tau, j, r)
    ah = R.alpha_hat64(T)
    g1, g2 = R.jump_tables(ref, ah)
    w = d.resample_walk(tau, j, r)
    assert w.g1.dtype == w.g2.dtype == torch.float32 and len(w.g1) == len(w.g2) == len(ref)
    np.testing.assert_allclose(w.g1.numpy(), g1, rtol=ULP2, atol=0)
    np.testing.assert_allclose(w.g2.numpy(), g2, rtol=ULP2, atol=0)
    ups = np.array([e[0] == "up" for e in ref])
    assert not g1[~ups].any() and not g2[~ups].any()
    if ups.any():
        assert (g1[ups] > 0).all() and (g1[ups] < 1).all() and (g2[ups] > 0).all()
        for a, b in ((g1, g2), (w.g1.numpy(), w.g2.numpy())):  # variance is preserved
            s = a[ups].astype(np.float64) ** 2 + b[ups].astype(np.float64) ** 2
            assert np.abs(s - 1).max() < ULP2
    # the jump composes the forward process: from level a to level b it is what noise_images does between them
    for (kind, frm, to, _), a in zip(ref, g1):
        if kind == "up":
            assert abs(float(a) - float(np.sqrt(np.prod(1.0 - _beta64(T)[frm + 1:to + 1])))) < 1e-7


def _beta64(T):
    return torch.linspace(1e-4, 0.02, T).double().numpy()


@pytest.mark.parametrize("S,j,r", CASES)
@pytest.mark.parametrize("eta", [0.0, 0.6])
def test_ddim_tables_of_the_walk(S, j, r, eta):
    d = _diff()
    tau = _tau(d, S)
    ref = R.walk(tau, j, r)
    want = R.ddim_tables(ref, R.alpha_hat64(T), eta)
    s = d._ddim(tau, eta, d.resample_walk(tau, j, r))
    got = d._walk_tables(s.walk, d._ddim_tables([e[1] for e in ref if e[0] == "down"], eta, "cpu", to=[e[2] for e in ref if e[0] == "down"]))
    for g, wnt in zip(got, want):
        np.testing.assert_allclose(g.numpy(), wnt.astype(np.float32), rtol=ULP2, atol=0)
    # steps: (k, a down entry, k where the entry draws): every up entry draws, a down entry where sigma != 0
    assert s.tau == [e[1] for e in ref] and s.t_first == tau[0]
    assert s.steps == [(k, e[0] == "down", k if (e[0] == "up" or want[4, k] != 0.0) else None) for k, e in enumerate(ref)]
    assert s.stats == d._ddim(tau, eta).stats
    # a revisited step has the coefficients of its first visit: they depend on (level from, level to) alone
    first = {}
    for k, e in enumerate(ref):
        if e[0] == "down":
            col = tuple(float(g[k]) for g in got)
            assert first.setdefault(e[3], col) == col


@pytest.mark.parametrize("S,j,r", CASES)
def test_dpmpp_c5_is_zero_after_every_up_entry(S, j, r):
    d = _diff()
    tau = _tau(d, S)
    ref = R.walk(tau, j, r)
    ah = R.alpha_hat64(T)
    want = R.dpmpp_tables(ref, ah, 2)
    w = d.resample_walk(tau, j, r)
    s = d._dpmpp(tau, 2, "time", w)
    down = [k for k, e in enumerate(ref) if e[0] == "down"]
    restart = [i for i, k in enumerate(down) if k and ref[k - 1][0] == "up"]
    got = d._walk_tables(w, d._dpmpp_tables([ref[k][1] for k in down], 2, "cpu", to=[ref[k][2] for k in down], restart=restart))
    for g, wnt in zip(got, want):
        np.testing.assert_allclose(g.numpy(), wnt.astype(np.float32), rtol=ULP2, atol=0)
    c5 = got[4].numpy()
    for k, e in enumerate(ref):
        if e[0] == "up":
            assert c5[k] == 0.0 and ref[k + 1][0] == "down" and c5[k + 1] == 0.0  # the jump itself, and the step after it
    assert c5[0] == 0.0 and c5[-1] == 0.0
    second = [k for k in down if k and ref[k - 1][0] == "down" and ref[k][2] != 0]
    assert all(c5[k] != 0.0 for k in second)  # ... and every other step is second order
    assert not np.any(d._walk_tables(w, d._dpmpp_tables([ref[k][1] for k in down], 1, "cpu", to=[ref[k][2] for k in down]))[4].numpy())
    assert s.steps == [(k, e[0] == "down", k if e[0] == "up" else None) for k, e in enumerate(ref)]  # only the jumps draw


def test_ddpm_walk_runs_in_table_form():
    d = _diff(8)
    w = d.resample_walk(range(7, 0, -1), 3, 2)
    s = d._ddpm(walk=w)
    ref = R.walk(range(7, 0, -1), 3, 2)
    assert s.tau == [e[1] for e in ref] == [7, 6, 5, 4, 7, 6, 5, 4, 3, 2, 1, 4, 3, 2, 1] and s.t_first == 7
    assert s.steps == [(k, e[0] == "down", k if (e[0] == "up" or e[1] > 1) else None) for k, e in enumerate(ref)]
    assert s.stats == d._ddpm().stats
    # with ``start`` the walk is built over start .. 1
    s5 = d._ddpm(start=5, walk=d.resample_walk(range(5, 0, -1), 2, 2))
    assert s5.t_first == 5 and s5.tau == [e[1] for e in R.walk(range(5, 0, -1), 2, 2)]


# ------------------------------------------------------------------------------------------------ the noise stream's tags
def test_the_four_tag_families_are_disjoint():
    assert N.TAG_WALK == R.TAG_WALK == 0xC0000000 and N.TAG_KNOWN == R.TAG_KNOWN
    assert (N.WALK_STEP, N.WALK_BLEND, N.WALK_JUMP) == (R.STEP, R.BLEND, R.JUMP) == (0, 1, 2)
    edge = lambda bound: [0, 1, 2, bound // 2, bound - 2, bound - 1]  # noqa: E731
    rng = np.random.default_rng(3)
    ks = edge(R.K_BOUND) + rng.integers(0, R.K_BOUND, 200).tolist()
    ts = edge(R.T_BOUND) + rng.integers(0, R.T_BOUND, 200).tolist()
    walk_tags = {R.tag(which, k) for which in (R.STEP, R.BLEND, R.JUMP) for k in ks}
    assert len(walk_tags) == 3 * len(set(ks))  # (which, k) -> tag is one to one
    families = {"t": set(ts), "known": {R.TAG_KNOWN | p for p in ts}, "stream": {0x80000000 | s for s in ts}, "walk": walk_tags}
    assert {name: {R.family(v) for v in tags} for name, tags in families.items()} == {"t": {0}, "known": {1}, "stream": {2}, "walk": {3}}
    assert all(0 <= v < 2 ** 32 for tags in families.values() for v in tags)
    with pytest.raises(AssertionError):
        R.tag(R.JUMP, R.K_BOUND)
    assert DM.WALK_MAX <= R.K_BOUND


def test_symbols_are_exported():
    lib = N.lib()
    for name in ("wd_forward_jump", "wd_walk_randn"):
        assert name in N.header_symbols() and getattr(lib, name) is not None


# ------------------------------------------------------------------------------------------------ argument handling
def _calls(d):
    return [(d.sampling, {}), (d.sampling_ddim, dict(steps=4)), (d.sampling_dpmpp, dict(steps=4)),
            (lambda m, vae, n, words, labels, args, **kw: d.sampling_phosc(m, vae, n, words, None, labels, args, **kw), {})]


def test_refusals_come_before_any_library_call(monkeypatch):
    d = _diff(8)
    args = make_args()
    m = UNetModel(args=args, **SMALL)
    mi = UNetModel(args=make_args(interpolation=True), **SMALL)
    n = 2
    labels = torch.tensor([1, 2], dtype=torch.int64)
    known = torch.zeros(n, 4, 4, 8)
    mask = torch.zeros(4, 8)
    mask[:, :4] = 1.0
    kept = dict(known=known, known_mask=mask)

    def no_library():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(N, "lib", no_library)
    bad = [(ValueError, m, dict(resample=2)),                                       # no mask: nothing to harmonise
           (ValueError, m, dict(resample=2, known=known, start=5)),                 # ``start`` alone keeps nothing either
           (ValueError, m, dict(resample=0, **kept)), (ValueError, m, dict(resample=-1, **kept)),
           (ValueError, m, dict(resample=2.0, **kept)), (ValueError, m, dict(resample=True, **kept)),
           (ValueError, m, dict(resample=2, jump=0, **kept)), (ValueError, m, dict(jump=0)), (ValueError, m, dict(resample=0)),
           (NotImplementedError, m, dict(resample=2, attention=True, **kept)),
           (NotImplementedError, m, dict(resample=2, attention=(5, 1), **kept)),
           (NotImplementedError, m, dict(resample=2, style_pairs=(1, 2), mix_rate=0.5, **kept)),
           (NotImplementedError, mi, dict(resample=2, mix_rate=0.5, **kept))]
    for call, extra in _calls(d):
        for exc, model, kw in bad:
            model.train()
            random.seed(5)
            torch.manual_seed(5)
            rs, ts = random.getstate(), torch.random.get_rng_state()
            d.last_stats = {}
            with pytest.raises(exc):
                call(model, None, n, ["ab", "cd"], labels, args, **kw, **extra)
            assert model.training and random.getstate() == rs and torch.equal(torch.random.get_rng_state(), ts), kw
            assert d.last_stats == {}
        # accepted calls get as far as the device check: resample=1 whatever else, and a resampled call with a mask
        for kw in (dict(resample=1, jump=3), dict(resample=1, attention=True), dict(resample=2, jump=2, **kept),
                   dict(resample=3, jump=1, start=5, **kept), dict(resample=2, attention=False, mix_rate=0.5, **kept)):
            with pytest.raises(N.NativeError, match="MI355X"):
                call(m, None, n, ["ab", "cd"], labels, args, **kw, **extra)
    # ``noise`` of a resampled call: one entry per walk entry
    z = [torch.zeros(n, 4, 4, 8)] * 7
    with pytest.raises(N.NativeError, match="MI355X"):
        d.sampling_ddim(m, None, n, ["ab", "cd"], labels, args, steps=4, eta=0.5, resample=2, jump=2, noise=z, **kept)
    for noise in (z[:4], z + z[:1]):
        with pytest.raises(ValueError, match="walk entry"):
            d.sampling_ddim(m, None, n, ["ab", "cd"], labels, args, steps=4, eta=0.5, resample=2, jump=2, noise=noise, **kept)
    with pytest.raises(ValueError, match="walk entry"):
        d.sampling(m, None, n, ["ab", "cd"], labels, args, resample=2, jump=3, noise=z, **kept)
    # the step-skipping sampler keeps no region
    m.train()
    with pytest.raises(NotImplementedError, match="sampling3"):
        d.sampling3(0, None, ["a"] * 2, None, m, m, None, 0, 1, 2, ["a"] * 2, labels, args, resample=2)
    assert m.training


def test_driver_flags():
    from worddiffusion_amd import driver
    base = ["--gt_train", "gt.txt", "--save_path", "out"]
    init = base + ["--init_latents", "c.npz", "--keep_cols", "0:12"]
    _, a = driver.parse_args(init + ["--resample", "3", "--jump", "4"])
    assert (a.resample, a.jump, a.keep_cols) == (3, 4, (0, 12))
    _, a = driver.parse_args(base)
    assert (a.resample, a.jump) == (1, 10)
    for bad in (base + ["--resample", "2"],                                              # nothing kept
                base + ["--init_latents", "c.npz", "--start", "5", "--resample", "2"],   # ``--start`` alone keeps nothing
                ["--lines", "l.txt", "--save_path", "out", "--resample", "2"],           # lines keep no region
                base + ["--skip_steps", "1", "--resample", "2"],
                init + ["--resample", "0"], init + ["--resample", "2", "--jump", "0"],
                init + ["--resample", "2", "--attn_maps", "m.npz"]):
        with pytest.raises(SystemExit):
            driver.parse_args(bad)
    d = _diff(8)
    with pytest.raises(ValueError, match="resample"):
        driver.regenerate(None, d, [], {}, make_args(), resample=2, rank=0, world=1)
    with pytest.raises(ValueError, match="resample"):
        driver.regenerate(None, d, [], {}, make_args(), known={}, keep_cols=(0, 4), skip_steps=True, resample=2, rank=0, world=1)
