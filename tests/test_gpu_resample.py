"""Resampling jumps (``resample=``, ``jump=``) on the GPU: ``wd_forward_jump`` and ``wd_walk_randn`` against their host
specification (``tests/_resample_ref.py``) on guarded operands, their draws against the Philox specification, their argument
checks, and the samplers around them - ``resample=1`` against the call without the argument, every entry of a resampled call
replayed through the C-ABI, graph replay against eager launches, sharding, the all-ones mask, one float64 trajectory, the
compositions with ``windows=``, writer-free guidance and ``start``, and the driver's command line.

Bounds: equality of bits wherever two fp32 evaluations of the same expression are compared; ``TOL`` of
``tests/test_gpu_noise.py`` (derived there, relative to the radius) for a device draw against the float64 specification, the
allowance ``tests/test_gpu_known.py`` gives ``wd_known_blend``; 1e-4 max-norm relative for the float64 trajectory, the bar
``tests/test_gpu_ddim.py`` holds its own float64 trajectory to."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ddpm_oracle as D  # noqa: E402
from oracle import unet_oracle as U  # noqa: E402
from tests import _ddim_ref as DR  # noqa: E402
from tests import _guard as G  # noqa: E402
from tests import _resample_ref as R  # noqa: E402
from tests._common import SMALL, make_args, max_rel  # noqa: E402
from tests.test_gpu_noise import _check, _ddpm_z  # noqa: E402  (the bound of a device draw and the step kernel's own draw)
from worddiffusion_amd import Diffusion, UNetModel  # noqa: E402
from worddiffusion_amd import _native as N  # noqa: E402
from worddiffusion_amd.synthetic import fill_module_, synthetic_tensor  # noqa: E402

DEV = "cuda:0"
HW = (32, 64)
SHAPE = (4, 4, 8)  # the latent of HW
NPIX = 128
T = 8
BIG = (3, 4 * 2 ** 18)  # more float4s than the 2048 x 256 threads a launch is capped at: the second grid-stride pass starts at row 2
SAMPLERS = ["ddpm", "ddim", "dpmpp"]


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _i32(*v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def _f32(a):
    return torch.tensor(np.asarray(a, dtype=np.float32), device=DEV)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _jump(x, batch, n, g1, g2, k, noise=None, seed=0, offset=0):
    return N.lib().wd_forward_jump(_ptr(x), batch, n, _ptr(g1), _ptr(g2), _ptr(k), _ptr(noise), seed, offset, _st())


def _fill(out, batch, n, seed, offset, which, k):
    return N.lib().wd_walk_randn(_ptr(out), batch, n, seed, offset, which, _ptr(k), _st())


def _walk_z(batch, n, seed, offset, which, k):
    out = torch.full((batch, n), float("nan"), device=DEV)
    N.check(_fill(out, batch, n, seed, offset, which, _i32(k)), "wd_walk_randn")
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------------------ 1. kernels against the specification
G1 = np.array([0.0, 0.96875, 0.25, 0.7071067811865476], dtype=np.float32)   # entry 0 is a down entry: its row is not an up entry's
G2 = np.array([0.0, 0.2480391, 0.96824584, 0.7071067811865476], dtype=np.float32)
CASES = [(b, n, k) for b in (1, 3) for n in (4, 1024) for k in (1, 3)] + [BIG + (2,)]


@pytest.mark.parametrize("drawn", [False, True], ids=["given-z", "drawn-z"])
@pytest.mark.parametrize("batch,n,k", CASES)
def test_forward_jump_bit_equal_to_the_specification(batch, n, k, drawn):
    seed, offset = 2 ** 32 + 77, 6
    g = torch.Generator().manual_seed(batch * 7 + n + k)
    x, z = (torch.randn(batch, n, generator=g) for _ in range(2))
    if drawn:  # the jump's own draw: what wd_walk_randn writes for (WD_WALK_JUMP, k), checked against Philox below
        z = _walk_z(batch, n, seed, offset, R.JUMP, k).cpu()
    xb, xv = G.guarded_flat(batch * n, torch.float32, device=DEV)
    xv.copy_(x.reshape(-1))
    zb, zv = G.guarded_flat(batch * n, torch.float32, device=DEV)
    if not drawn:
        zv.copy_(z.reshape(-1))
    g1, g2 = _f32(G1), _f32(G2)
    rc = _jump(xv, batch, n, g1, g2, _i32(k), None if drawn else zv, seed, offset)
    torch.cuda.synchronize()
    assert rc == N.WD_OK
    G.assert_untouched(xb, xv, "x")
    G.assert_untouched(zb, zv, "noise")
    G.assert_finite(xv, "x")
    if not drawn:
        assert torch.equal(zv.cpu().reshape(batch, n), z), "noise was written"
    want = R.forward_jump(x.numpy(), G1[k], G2[k], z.numpy())
    assert _same_bits(xv.reshape(batch, n), torch.from_numpy(want))
    assert not torch.equal(xv.cpu().reshape(batch, n), x)


@pytest.mark.parametrize("batch,n,k", CASES)
def test_walk_randn_equals_the_philox_specification_inside_its_window(batch, n, k):
    seed, offset = 2 ** 32 + 77, 6
    for which in ((R.STEP, R.BLEND, R.JUMP) if n < BIG[1] else (R.BLEND,)):
        buf, view = G.guarded_flat(batch * n, torch.float32, device=DEV)
        assert _fill(view, batch, n, seed, offset, which, _i32(k)) == N.WD_OK
        torch.cuda.synchronize()
        G.assert_untouched(buf, view, "out")
        _check(view.reshape(batch, n), R.draw(batch, n, seed, offset, which, k, with_r=True), f"wd_walk_randn which={which} k={k}")


# ------------------------------------------------------------------------------------------------ 2. the draws
@pytest.mark.parametrize("k", [0, 5, 2 ** 26 - 1])
def test_draws_equal_the_philox_specification(k):
    seed, offset = 2 ** 32 + 77, 6
    for which in (R.STEP, R.BLEND, R.JUMP):
        _check(_walk_z(3, 128, seed, offset, which, k), R.draw(3, 128, seed, offset, which, k, with_r=True), f"which={which} k={k}")
    # the jump's own draw (x = 0, g1 = 0, g2 = 1 leaves z in x) is the WD_WALK_JUMP fill, bit for bit
    x = torch.zeros(3, 128, device=DEV)
    tab = torch.zeros(8, device=DEV)
    one = torch.ones(8, device=DEV)
    N.check(_jump(x, 3, 128, tab, one, _i32(5), None, seed, offset), "wd_forward_jump")
    torch.cuda.synchronize()
    assert torch.equal(x, _walk_z(3, 128, seed, offset, R.JUMP, 5))


def test_every_key_word_of_the_draw_is_live():
    base = _walk_z(3, 128, 77, 6, R.STEP, 5)
    assert torch.equal(base, _walk_z(3, 128, 77, 6, R.STEP, 5))
    assert not torch.equal(base, _walk_z(3, 128, 77, 6, R.STEP, 4))             # k: a second visit of a level draws afresh
    assert not torch.equal(base, _walk_z(3, 128, 77, 6, R.BLEND, 5))            # which
    assert not torch.equal(base, _walk_z(3, 128, 77, 6, R.JUMP, 5))
    assert not torch.equal(_walk_z(3, 128, 77, 6, R.BLEND, 5), _walk_z(3, 128, 77, 6, R.JUMP, 5))
    assert not torch.equal(base, _walk_z(3, 128, 78, 6, R.STEP, 5))             # seed
    assert not torch.equal(base, _walk_z(3, 128, 2 ** 32 + 77, 6, R.STEP, 5))   # its high word
    assert not torch.equal(base[0], base[1]) and not torch.equal(base[:, :4], base[:, 4:8])  # row, element counter
    shifted = _walk_z(3, 128, 77, 7, R.STEP, 5)                                 # sample_offset: rows 7, 8, 9
    assert torch.equal(shifted[:2], base[1:]) and not torch.equal(shifted[2], base[2])
    assert not torch.equal(base, _walk_z(3, 128, 77, 2 ** 32 + 6, R.STEP, 5))   # high word of the row
    # a tag family of its own: not the step kernel's draw at t = 5, not any wd_randn stream at the same key
    assert not torch.equal(base, _ddpm_z(3, 128, 5, 77, 6))
    for stream_id in (0, 1, 2, 3, 4, 5):
        r = torch.empty(3, 128, device=DEV)
        N.check(N.lib().wd_randn(r.data_ptr(), 3, 128, 77, 6, stream_id, _st()), "wd_randn")
        torch.cuda.synchronize()
        assert not torch.equal(base, r), stream_id


# ------------------------------------------------------------------------------------------------ 3. argument checks
def test_einval_launches_nothing():
    batch, n = 2, 64
    g = torch.Generator().manual_seed(4)
    buf, x = G.guarded_flat(batch * n, torch.float32, device=DEV)
    before = torch.randn(batch * n, generator=g).to(DEV)
    x.copy_(before)
    z = torch.rand(batch * n + 4, generator=g).to(DEV)
    g1, g2, k = _f32(G1), _f32(G2), _i32(1)
    off = lambda v: v[1:1 + batch * n]  # noqa: E731  (4 bytes past a 16-byte boundary)
    assert off(z).data_ptr() % 16 == 4
    xbuf = torch.zeros(batch * n + 4, device=DEV)
    good = dict(x=x, batch=batch, n=n, g1=g1, g2=g2, k=k, noise=z[:-4])
    for bad in (dict(x=None), dict(g1=None), dict(g2=None), dict(k=None), dict(n=62), dict(n=0), dict(batch=0), dict(x=off(xbuf)),
                dict(noise=off(z))):
        assert _jump(**dict(good, **bad)) == N.WD_EINVAL, sorted(bad)
    goodf = dict(out=x, batch=batch, n=n, seed=1, offset=0, which=0, k=k)
    for bad in (dict(out=None), dict(k=None), dict(n=62), dict(n=0), dict(batch=0), dict(out=off(xbuf)), dict(which=3), dict(which=-1)):
        assert _fill(**dict(goodf, **bad)) == N.WD_EINVAL, sorted(bad)
    torch.cuda.synchronize()
    G.assert_untouched(buf, x, "x")
    assert torch.equal(x, before) and not xbuf.any()
    for form in (dict(), dict(noise=None)):  # and the call itself is good
        assert _jump(**dict(good, **form)) == N.WD_OK
    assert _fill(**goodf) == N.WD_OK
    torch.cuda.synchronize()
    G.assert_untouched(buf, x, "x")
    assert not torch.equal(x, before)


# ------------------------------------------------------------------------------------------------ the samplers
def _model(cls, cfg, seed, **args_kw):
    return fill_module_(cls(args=make_args(device=DEV, **args_kw), **cfg), seed).to(DEV).eval()


@pytest.fixture(scope="module")
def setup():
    args = make_args(device=DEV)
    m = _model(UNetModel, SMALL, 5)
    diff = Diffusion(noise_steps=T, img_size=HW, args=args)
    g = torch.Generator().manual_seed(6)
    known = torch.randn(4, *SHAPE, generator=g) * 0.8
    labels = torch.tensor([1, 7, 3, 9], dtype=torch.int64)
    words = ["MOVE", "a", "Zebra", "quilt"]
    cols = torch.zeros(SHAPE[1], SHAPE[2])
    cols[:, :4] = 1.0          # the first half of the columns is kept
    soft = cols.clone()
    soft[:, 4] = 0.5           # ... and one column feathers
    return m, diff, args, labels, words, known, cols, soft


def _call(diff, which, m, n, words, labels, args, **kw):
    """One call of a sampler on the first n rows; the short schedules the tests share: 7 / 4 / 4 steps of T = 8."""
    if which == "ddpm":
        return diff.sampling(m, None, n, words[:n], labels[:n], args, **kw)
    if which == "ddim":
        return diff.sampling_ddim(m, None, n, words[:n], labels[:n], args, steps=4, **kw)
    return diff.sampling_dpmpp(m, None, n, words[:n], labels[:n], args, steps=4, spacing="time", **kw)


def _plain_tau(which, start=None):
    first = T - 1 if start is None else start
    return list(range(first, 0, -1)) if which == "ddpm" else [t for t in (7, 5, 3, 1) if t <= first]


# ------------------------------------------------------------------------------------------------ 4. resample=1 is the plain call
@pytest.mark.parametrize("which", SAMPLERS)
def test_resample_1_is_the_call_without_the_argument(setup, which):
    m, diff, args, labels, words, known, cols, soft = setup
    n = 3
    eta = dict(eta=0.5) if which == "ddim" else {}
    for kw in (dict(), dict(known=known[:n], known_mask=soft), dict(known=known[:n], known_mask=soft, start=5, known_noise="fresh")):
        a = _call(diff, which, m, n, words, labels, args, seed=17, sample_offset=2, **eta, **kw)
        sa = dict(diff.last_stats)
        b = _call(diff, which, m, n, words, labels, args, seed=17, sample_offset=2, resample=1, jump=2, **eta, **kw)
        assert _same_bits(a, b) and diff.last_stats == sa, kw
        assert (sa["resample"], sa["jump"], sa["walk"], sa["graph"]) == (1, None, sa["steps"], True)
    # ... and r > 1 with a jump that spans the schedule has no up entry, but draws by walk entry: another sample of the same law
    c = _call(diff, which, m, n, words, labels, args, seed=17, sample_offset=2, resample=2, jump=7, known=known[:n], known_mask=soft, **eta)
    st = diff.last_stats
    assert (st["resample"], st["jump"], st["walk"], st["model_calls"]) == (2, 7, st["steps"], st["steps"])
    assert _same_bits(c[..., :4], known[:n][..., :4]) and torch.isfinite(c).all()


# ------------------------------------------------------------------------------------------------ 5. every entry through the C-ABI
def _down_tables(diff, which, ref, eta):
    """The step kernel's tables over all walk entries, from the library's own per-(from, to) table functions (their values are held
    to the specification by ``tests/test_resample_host.py``); DDPM reads its tables by t."""
    if which == "ddpm":
        return diff._step_tables(DEV)
    down = [k for k, e in enumerate(ref) if e[0] == "down"]
    frm, to = [ref[k][1] for k in down], [ref[k][2] for k in down]
    if which == "ddim":
        tabs = diff._ddim_tables(frm, eta, "cpu", to=to)
    else:
        tabs = diff._dpmpp_tables(frm, 2, "cpu", to=to, restart=[i for i, k in enumerate(down) if k and ref[k - 1][0] == "up"])
    out = []
    for t in tabs:
        full = torch.zeros(len(ref))
        full[down] = t
        out.append(full.to(DEV))
    return out


def _replay(diff, which, ref, states, preds, n, npix, seed, offset, x0, mask, mode, eta=0.0, noise=None, line_pred=None, guided=None):
    """Replays every walk entry on the state recorded before it: a down entry as fill, step, blend, an up entry as the jump; the
    result must be the next recorded state, bit for bit.  ``line_pred(p)`` picks the prediction(s) the update reads out of what
    ``record_pred`` received; ``guided``: the scale of a two-prediction step."""
    lib = N.lib()
    W = len(ref)
    assert len(states) == W + 1 and len(preds) == sum(e[0] == "down" for e in ref)
    ah = R.alpha_hat64(T)
    g1, g2 = (_f32(t) for t in R.jump_tables(ref, ah))
    tabs = _down_tables(diff, which, ref, eta)
    sigma = None if which != "ddim" else tabs[4].cpu().tolist()
    tau_dev = _i32(*[e[1] for e in ref])
    sa, sb = diff._noise_tables(DEV)
    keps = None
    if mode == "fixed":
        keps = torch.empty(n, npix, device=DEV)
        N.check(lib.wd_randn(keps.data_ptr(), n, npix, seed, offset, N.STREAM_KNOWN, _st()), "wd_randn")
    x0_prev = torch.empty(n, npix, device=DEV)
    d = 0
    for k, (kind, frm, to, _) in enumerate(ref):
        x = states[k].clone()
        k_dev, t_dev = _i32(k), _i32(frm)
        given = None if noise is None else noise[k].to(DEV).contiguous()
        if kind == "up":
            N.check(_jump(x, n, npix, g1, g2, k_dev, given, seed, offset), "wd_forward_jump")
            torch.cuda.synchronize()
            assert _same_bits(x, states[k + 1]), (which, k, "up")
            assert not torch.equal(x, states[k])
            continue
        p = preds[d]
        d += 1
        first, second, guided_pred = (p[0], None, None) if line_pred is None else line_pred(p)
        draws = frm > 1 if which == "ddpm" else (sigma[k] != 0.0 if which == "ddim" else False)
        z = None
        if draws:
            z = given if given is not None else _walk_z(n, npix, seed, offset, R.STEP, k)
        scale = 0.0 if guided is None else guided
        eg = torch.empty(n, npix, device=DEV) if guided is not None else None
        if which == "ddpm":
            N.check(lib.wd_ddpm_step(x.data_ptr(), first.data_ptr(), n, npix, *(c.data_ptr() for c in tabs), t_dev.data_ptr(), _ptr(z),
                                     seed, offset, _st()), "wd_ddpm_step")
        elif which == "ddim":
            N.check(lib.wd_ddim_step(x.data_ptr(), first.data_ptr(), _ptr(second), scale, _ptr(eg), n, npix, *(c.data_ptr() for c in tabs),
                                     k_dev.data_ptr(), t_dev.data_ptr(), _ptr(z), seed, offset, _st()), "wd_ddim_step")
        else:
            N.check(lib.wd_dpmpp_step(x.data_ptr(), first.data_ptr(), _ptr(second), scale, _ptr(eg), x0_prev.data_ptr(), n, npix,
                                      *(c.data_ptr() for c in tabs), k_dev.data_ptr(), _st()), "wd_dpmpp_step")
        torch.cuda.synchronize()
        if guided is not None:
            assert _same_bits(eg.reshape(guided_pred.shape), guided_pred)
        assert not torch.equal(x, states[k + 1]), (k, "the blend changed nothing")
        kz = keps if mode == "fixed" else _walk_z(n, npix, seed, offset, R.BLEND, k)
        N.check(lib.wd_known_blend(x.data_ptr(), x0.data_ptr(), mask.data_ptr(), n, npix, sa.data_ptr(), sb.data_ptr(), t_dev.data_ptr(),
                                   k_dev.data_ptr(), tau_dev.data_ptr(), W, kz.data_ptr(), seed, offset, _st()), "wd_known_blend")
        torch.cuda.synchronize()
        assert _same_bits(x, states[k + 1]), (which, mode, k, "down", frm, to)


REPLAYS = [("ddpm", "fresh", {}), ("ddim", "fresh", dict(eta=0.5)), ("ddim", "fixed", {}), ("dpmpp", "fixed", {}),
           ("dpmpp", "fresh", dict(known_noise="fresh"))]


@pytest.mark.parametrize("which,mode,extra", REPLAYS, ids=[f"{w}-{md}" for w, md, _ in REPLAYS])
def test_every_entry_of_a_resampled_call_replays_through_the_c_abi(setup, which, mode, extra):
    m, diff, args, labels, words, known, cols, soft = setup
    n, seed, offset = 3, 41, 5
    rec, preds = [], []
    out = _call(diff, which, m, n, words, labels, args, seed=seed, sample_offset=offset, known=known[:n], known_mask=soft,
                resample=2, jump=2, record=rec, record_pred=preds, **extra)
    st = diff.last_stats
    ref = R.walk(_plain_tau(which), 2, 2)
    downs, ups = R.counts(len(_plain_tau(which)), 2, 2)
    assert ups >= 1 and (st["resample"], st["jump"], st["walk"], st["model_calls"]) == (2, 2, downs + ups, downs)
    assert (st["known"], st["known_noise"], st["graph"], st["steps"]) == (True, mode, False, len(_plain_tau(which)))
    assert len(rec) == downs + ups and len(preds) == downs
    x0 = known[:n].reshape(n, -1).to(DEV)
    mask = soft.expand(n, *SHAPE).reshape(n, -1).contiguous().to(DEV)
    _replay(diff, which, ref, rec + [out], preds, n, NPIX, seed, offset, x0, mask, mode, eta=extra.get("eta", 0.0))
    assert torch.equal(out.reshape(n, *SHAPE)[..., :4].cpu(), known[:n][..., :4])
    # the second visit of a stretch is not the first: the jump drew, and so did the steps and blends that draw
    first_up = [e[0] for e in ref].index("up")
    assert not torch.equal(rec[first_up + 1], rec[first_up - 2]) and not torch.equal(rec[first_up + 3], rec[first_up])


@pytest.mark.parametrize("which", SAMPLERS)
def test_a_revisited_level_reads_its_own_film_rows(setup, which):
    """The FiLM table of a resampled call is indexed by the walk entry: the prediction of every down entry is the model's forward on
    the recorded state at the level the entry starts from.  Bound: the two are fp32 evaluations of one function through different
    launch plans and agree far inside 1e-3 max-norm relative (whole trajectories are held to 1e-4 against float64), while the rows of
    another level change the prediction at order one (measured on an MI355X: 0 against 4.3e-2 at the nearest)."""
    m, diff, args, labels, words, known, cols, soft = setup
    n = 3
    rec, preds = [], []
    _call(diff, which, m, n, words, labels, args, seed=3, known=known[:n], known_mask=soft, resample=2, jump=2, record=rec, record_pred=preds)
    m.eval()
    ctx = diff._text_features(words[:n], n).to(DEV)
    down = [(k, e[1]) for k, e in enumerate(R.walk(_plain_tau(which), 2, 2)) if e[0] == "down"]
    errs, wrong = [], []
    with torch.no_grad():
        for (k, t), p in zip(down, preds):
            fwd = lambda level: m(rec[k], timesteps=torch.full((n,), level, dtype=torch.int64, device=DEV), context=ctx,  # noqa: E731
                                  y=labels[:n].to(DEV))
            errs.append(max_rel(p[0].cpu(), fwd(t).cpu()))
            wrong.append(max_rel(p[0].cpu(), fwd(t - 1 if t > 1 else t + 1).cpu()))
    print(f"{which}: prediction against the forward at the entry's level {max(errs):.2e}, at a neighbouring level {min(wrong):.2e}")
    assert max(errs) < 1e-3 < min(wrong)


def test_given_noise_is_indexed_by_walk_entry(setup):
    """``noise[k]`` is the one draw entry k makes: the step's z of a down entry, the jump's z of an up entry - replayed as such."""
    m, diff, args, labels, words, known, cols, soft = setup
    n, seed, offset = 3, 41, 5
    ref = R.walk(_plain_tau("ddim"), 2, 2)
    g = torch.Generator().manual_seed(11)
    noise = [torch.randn(n, *SHAPE, generator=g) for _ in ref]
    rec, preds = [], []
    out = _call(diff, "ddim", m, n, words, labels, args, seed=seed, sample_offset=offset, known=known[:n], known_mask=soft, eta=0.5,
                resample=2, jump=2, noise=noise, record=rec, record_pred=preds)
    x0 = known[:n].reshape(n, -1).to(DEV)
    mask = soft.expand(n, *SHAPE).reshape(n, -1).contiguous().to(DEV)
    _replay(diff, "ddim", ref, rec + [out], preds, n, NPIX, seed, offset, x0, mask, "fresh", eta=0.5, noise=noise)
    # through the graph as well
    again = _call(diff, "ddim", m, n, words, labels, args, seed=seed, sample_offset=offset, known=known[:n], known_mask=soft, eta=0.5,
                  resample=2, jump=2, noise=noise)
    assert diff.last_stats["graph"] and _same_bits(again, out)


# ------------------------------------------------------------------------------------------------ 6. graph == eager, sharding
@pytest.mark.parametrize("which", SAMPLERS)
def test_graph_replay_equals_eager(setup, which):
    m, diff, args, labels, words, known, cols, soft = setup
    n = 3
    eta = dict(eta=0.5) if which == "ddim" else {}
    for kw in (dict(known_mask=soft, resample=2, jump=2), dict(known_mask=soft, resample=3, jump=1, known_noise="fresh"),
               dict(known_mask=cols, resample=2, jump=3, start=6, known_noise="fixed")):
        outs = []
        for use_graph in (True, False):
            outs.append(_call(diff, which, m, n, words, labels, args, seed=23, sample_offset=1, known=known[:n], use_graph=use_graph,
                              **eta, **kw))
            assert diff.last_stats["graph"] == use_graph
        assert _same_bits(outs[0], outs[1]), kw
        assert torch.isfinite(outs[0]).all() and _same_bits(outs[0][..., :4], known[:n][..., :4])


@pytest.mark.parametrize("which", SAMPLERS)
def test_a_resampled_call_is_keyed_by_the_global_row(setup, which):
    m, diff, args, labels, words, known, cols, soft = setup
    eta = dict(eta=0.5) if which == "ddim" else {}
    kw = dict(seed=29, known_mask=soft, known_noise="fresh", resample=2, jump=2, **eta)
    whole = _call(diff, which, m, 4, words, labels, args, sample_offset=0, known=known, **kw)
    lo = _call(diff, which, m, 2, words, labels, args, sample_offset=0, known=known[:2], **kw)
    hi = _call(diff, which, m, 2, words[2:], labels[2:], args, sample_offset=2, known=known[2:], **kw)
    assert _same_bits(whole[:2], lo) and _same_bits(whole[2:], hi)
    assert not torch.equal(whole[..., 5:], _call(diff, which, m, 4, words, labels, args, sample_offset=0, known=known,
                                                 **dict(kw, seed=30))[..., 5:])
    assert not torch.equal(whole[0], whole[1])


# ------------------------------------------------------------------------------------------------ 7. masks
@pytest.mark.parametrize("which", SAMPLERS)
def test_a_mask_of_all_ones_returns_known(setup, which):
    m, diff, args, labels, words, known, cols, soft = setup
    full = _call(diff, which, m, 3, words, labels, args, seed=17, known=known[:3], known_mask=torch.ones(SHAPE[1:]), resample=2, jump=2)
    assert _same_bits(full, known[:3]) and diff.last_stats["graph"]
    got = _call(diff, which, m, 3, words, labels, args, seed=17, known=known[:3], known_mask=cols, resample=2, jump=2)
    plain = _call(diff, which, m, 3, words, labels, args, seed=17, known=known[:3], known_mask=cols)
    assert _same_bits(got[..., :4], known[:3][..., :4]) and torch.isfinite(got).all()
    assert not torch.equal(got[..., 4:], plain[..., 4:]) and not torch.equal(got[..., 4:].cpu(), known[:3][..., 4:])


# ------------------------------------------------------------------------------------------------ 8. one float64 trajectory
def test_resampled_ddim_trajectory_matches_float64_oracle():
    """DDIM, eta = 0, T = 8, 4 steps, j = 2, r = 2, given ``noise`` and ``known_noise``, the first half of the columns kept: every
    state against the CPU oracle UNet with update, blend and jump in float64, to the bar of
    ``test_gpu_ddim.test_ddim_trajectory_matches_float64_oracle``."""
    S, n, seed = 4, 3, 9
    args = make_args(device=DEV)
    m = _model(UNetModel, SMALL, seed)
    diff = Diffusion(noise_steps=T, img_size=HW, args=args)
    tau = diff.ddim_timesteps(S)
    assert tau == [7, 5, 3, 1]
    ref = R.walk(tau, 2, 2)
    g = torch.Generator().manual_seed(3)
    x_T, known, E = (torch.randn(n, *SHAPE, generator=g) for _ in range(3))
    noise = [torch.randn(n, *SHAPE, generator=g) for _ in ref]
    mask = torch.zeros(SHAPE[1:])
    mask[:, :4] = 1.0
    labels = torch.tensor([1, 7, 10], dtype=torch.int64)
    word = "Moving"
    rec = []
    out = diff.sampling_ddim(m, None, n, word, labels, args, steps=S, eta=0.0, x_T=x_T, known=known, known_mask=mask, known_noise=E,
                             resample=2, jump=2, noise=noise, record=rec)
    assert (diff.last_stats["model_calls"], diff.last_stats["walk"], diff.last_stats["known_noise"]) == (6, 7, "fixed")
    sd = {k: torch.from_numpy(synthetic_tensor(k, s, seed)).double() for k, s in U.state_dict_shapes(SMALL, "base")}
    orc = U.UNetOracle(SMALL, sd, "base", False)
    ctx = torch.tensor([D.label_padding(word)] * n, dtype=torch.int64)
    ah = DR.alpha_hat64(T)
    c = torch.from_numpy(R.ddim_tables(ref, ah.numpy(), 0.0))
    x, x0, z, mk = x_T.double(), known.double(), E.double(), mask.double()
    states = []
    with torch.no_grad():
        for k, (kind, frm, to, _) in enumerate(ref):
            states.append(x.clone())
            if kind == "up":
                x = R.forward_jump64(x, ah.numpy(), frm, to, noise[k].double())
                continue
            eps = orc(x, torch.full((n,), frm, dtype=torch.int64), ctx, labels, None).double()
            x = DR.step(c, k, x, eps)
            kv = x0 if to == 0 else torch.sqrt(ah[to]) * x0 + torch.sqrt(1 - ah[to]) * z
            x = x + mk * (kv - x)
    xs = torch.stack([r.cpu() for r in rec] + [out.cpu()])
    ref_xs = torch.stack(states + [x])
    assert xs.shape == ref_xs.shape == (len(ref) + 1, n, *SHAPE)
    errs = [max_rel(xs[k], ref_xs[k]) for k in range(len(ref) + 1)]
    print(f"resampled ddim trajectory: max_rel per state {['%.2e' % e for e in errs]}")
    assert max(errs) < 1e-4
    assert torch.equal(out[..., :4].cpu(), known[..., :4])


# ------------------------------------------------------------------------------------------------ 9. composition
def test_a_resampled_line_call_replays_entry_by_entry():
    """``windows=`` with K = 2: update, blend and jump act on the line latent; the window predictions blend into the line
    prediction the update reads."""
    hw, C, H, WM = (64, 64), 4, 8, 8
    args = make_args(device=DEV)
    m = _model(UNetModel, SMALL, 5)
    diff = Diffusion(noise_steps=T, img_size=hw, args=args)
    n, Kw, seed, offset = 2, 2, 41, 5
    lw = diff.line_windows(n, Kw, overlap=3, feather=2)
    wl = lw.width
    npix = C * H * wl
    g = torch.Generator().manual_seed(6)
    known = torch.randn(n, C, H, wl, generator=g) * 0.8
    soft = torch.zeros(H, wl)
    soft[:, :6] = 1.0
    soft[:, 6] = 0.5  # kept columns reach into the overlap
    lines = [["MOVE", "a"], ["quilt", "Moving"]]
    labels = torch.tensor([1, 7], dtype=torch.int64)
    rec, preds = [], []
    out = diff.sampling_ddim(m, None, n, lines, labels, args, steps=4, eta=0.5, seed=seed, sample_offset=offset, known=known,
                             known_mask=soft, windows=lw, resample=2, jump=2, record=rec, record_pred=preds)
    st = diff.last_stats
    assert (st["windows"], st["model_batch"], st["walk"], st["model_calls"], st["graph"]) == (Kw, n * Kw, 7, 6, False)
    ref = R.walk([7, 5, 3, 1], 2, 2)
    off_dev, wn_dev = lw.offsets.to(DEV), lw.wn.to(DEV)

    def line_pred(p):
        assert len(p) == 2 and p[0].shape == (n * Kw, C, H, WM) and p[1].shape == (n, C, H, wl)
        e0 = torch.empty(n, npix, device=DEV)
        N.check(N.lib().wd_window_blend(p[0].data_ptr(), None, wn_dev.data_ptr(), off_dev.data_ptr(), n, Kw, C, H, WM, wl, e0.data_ptr(), None,
                                        _st()), "wd_window_blend")
        torch.cuda.synchronize()
        assert _same_bits(e0.reshape(n, C, H, wl), p[1])
        return e0, None, None
    x0 = known.reshape(n, -1).to(DEV)
    mask = soft.expand(n, C, H, wl).reshape(n, -1).contiguous().to(DEV)
    _replay(diff, "ddim", ref, rec + [out], preds, n, npix, seed, offset, x0, mask, "fresh", eta=0.5, line_pred=line_pred)
    assert out.shape == (n, C, H, wl) and torch.equal(out[..., :6].cpu(), known[..., :6])
    graph = diff.sampling_ddim(m, None, n, lines, labels, args, steps=4, eta=0.5, seed=seed, sample_offset=offset, known=known,
                               known_mask=soft, windows=lw, resample=2, jump=2)
    assert diff.last_stats["graph"] and _same_bits(graph, out)


def test_a_resampled_guided_call_replays_entry_by_entry(setup):
    """Writer-free guidance: rows and FiLM are per entry; a down entry is two forwards and the guided update."""
    m, diff, args, labels, words, known, cols, soft = setup
    n, seed, offset, scale = 3, 41, 5, 3.0
    rec, preds = [], []
    out = _call(diff, "ddim", m, n, words, labels, args, seed=seed, sample_offset=offset, known=known[:n], known_mask=soft, eta=0.5,
                guidance="writer_free", cfg_scale=scale, resample=2, jump=2, record=rec, record_pred=preds)
    st = diff.last_stats
    assert (st["forwards_per_step"], st["guidance"], st["walk"], st["model_calls"]) == (2, "writer_free", 7, 12)
    ref = R.walk([7, 5, 3, 1], 2, 2)

    def line_pred(p):
        assert len(p) == 3 and not torch.equal(p[0], p[1])
        return p[0], p[1], p[2]
    x0 = known[:n].reshape(n, -1).to(DEV)
    mask = soft.expand(n, *SHAPE).reshape(n, -1).contiguous().to(DEV)
    _replay(diff, "ddim", ref, rec + [out], preds, n, NPIX, seed, offset, x0, mask, "fresh", eta=0.5, line_pred=line_pred, guided=scale)
    graph = _call(diff, "ddim", m, n, words, labels, args, seed=seed, sample_offset=offset, known=known[:n], known_mask=soft, eta=0.5,
                  guidance="writer_free", cfg_scale=scale, resample=2, jump=2)
    assert diff.last_stats["graph"] and _same_bits(graph, out)


@pytest.mark.parametrize("which,start,level", [("ddpm", 5, 5), ("ddim", 6, 5), ("dpmpp", 6, 5)])
def test_start_visits_the_walk_of_the_retained_schedule(setup, which, start, level):
    m, diff, args, labels, words, known, cols, soft = setup
    n, seed, offset = 3, 13, 4
    rec, preds = [], []
    out = _call(diff, which, m, n, words, labels, args, seed=seed, sample_offset=offset, known=known[:n], known_mask=soft, start=start,
                resample=2, jump=2, record=rec, record_pred=preds)
    st = diff.last_stats
    tau = _plain_tau(which, level)
    ref = R.walk(tau, 2, 2)
    downs, ups = R.counts(len(tau), 2, 2)
    assert (st["start"], st["steps"], st["walk"], st["model_calls"]) == (level, len(tau), downs + ups, downs) and len(rec) == downs + ups
    assert st.get("timesteps") == (None if which == "ddpm" else tau)
    # the first state is ``known`` noised to the level; every entry replays, so the levels visited are the walk's
    eps = torch.empty(n, *SHAPE, device=DEV)
    N.check(N.lib().wd_randn(eps.data_ptr(), n, NPIX, seed, offset, N.STREAM_KNOWN, _st()), "wd_randn")
    want, _ = diff.noise_images(known[:n].to(DEV), torch.full((n,), level, dtype=torch.int64), eps=eps)
    assert _same_bits(rec[0], want)
    x0 = known[:n].reshape(n, -1).to(DEV)
    mask = soft.expand(n, *SHAPE).reshape(n, -1).contiguous().to(DEV)
    _replay(diff, which, ref, rec + [out], preds, n, NPIX, seed, offset, x0, mask, st["known_noise"])


def test_model_state_after_a_resampled_call(setup):
    m, diff, args, labels, words, known, cols, soft = setup
    m.eval()
    out = diff.sampling_dpmpp(m, None, 3, words[:3], labels[:3], args, steps=3, known=known[:3], known_mask=cols, resample=2, jump=1)
    assert m.training and out.shape == (3, *SHAPE) and diff.last_stats["walk"] == 3 + 2 + 2
    m.eval()


# ------------------------------------------------------------------------------------------------ 10. driver
def test_driver_command_line_with_resample(golden_dir, tmp_path, monkeypatch):
    from worddiffusion_amd import driver
    from worddiffusion_amd.latents import LatentCache, save_latent_cache
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    gt = tmp_path / "gt.txt"
    lines = [ln for ln in open(os.path.join(golden_dir, "gt_samples.txt")).read().splitlines() if ln.strip()]
    gt.write_text("\n".join([ln for ln in lines if not ln.startswith("#")][:3]) + "\n")
    rows = driver.read_gt(str(gt))
    g = torch.Generator().manual_seed(12)
    latents = {image + ".png": torch.randn(4, 8, 32, generator=g) for _, image, _ in rows}
    cache = str(tmp_path / "latents.npz")
    save_latent_cache(cache, latents)
    args = make_args(device=DEV)
    kw = dict(image_size=(64, 256), in_channels=4, model_channels=64, out_channels=4, num_res_blocks=1, attention_resolutions=(1, 1),
              channel_mult=(1, 1), num_heads=2, num_classes=339, context_dim=64, vocab_size=53, max_seq_len=10)
    m = fill_module_(UNetModel(args=args, **kw), 17)
    os.makedirs(tmp_path / "run" / "models")
    torch.save(m.state_dict(), tmp_path / "run" / "models" / "ema_ckpt.pt")
    out = tmp_path / "out"
    base = ["--gt_train", str(gt), "--models_path", str(tmp_path / "run"), "--save_path", str(out), "--writer_dict",
            str(tmp_path / "writers.json"), "--batch_size", "2", "--emb_dim", "64", "--num_heads", "2", "--noise_steps", "11",
            "--seed", "5", "--init_latents", cache, "--keep_cols", "0:12", "--sampler", "ddim", "--ddim_steps", "4",
            "--resample", "2", "--jump", "2"]
    driver.main(base)
    assert sorted(os.listdir(out / "images")) == sorted(r[1] + ".npy" for r in rows)
    m = m.to(DEV).eval().requires_grad_(False)
    diff = Diffusion(noise_steps=11, img_size=(64, 256), args=args)
    wr = driver.writer_dict(rows, str(tmp_path / "writers.json"))
    mask = driver.keep_cols_mask((0, 12), 8, 32)
    known = LatentCache(cache)
    for b0 in (0, 2):  # the driver's batches of 2: rows 0-1, row 2
        chunk = rows[b0:b0 + 2]
        labels = torch.tensor([wr[s] for s, _, _ in chunk], dtype=torch.int64)
        kn = torch.stack([known[image + ".png"] for _, image, _ in chunk])
        ref = diff.sampling_ddim(m, None, len(chunk), [w for _, _, w in chunk], labels, args, steps=4, seed=5, sample_offset=b0,
                                 known=kn, known_mask=mask, resample=2, jump=2).cpu()
        assert (diff.last_stats["walk"], diff.last_stats["model_calls"], diff.last_stats["resample"]) == (7, 6, 2)
        plain = diff.sampling_ddim(m, None, len(chunk), [w for _, _, w in chunk], labels, args, steps=4, seed=5, sample_offset=b0,
                                   known=kn, known_mask=mask).cpu()
        for (_, image, _), r, k0, pl in zip(chunk, ref, kn, plain):
            got = np.load(out / "images" / f"{image}.npy")
            assert np.array_equal(got, r.numpy()), image
            assert np.array_equal(got[:, :, :12], k0.numpy()[:, :, :12]) and not np.array_equal(got[:, :, 12:], pl.numpy()[:, :, 12:])
