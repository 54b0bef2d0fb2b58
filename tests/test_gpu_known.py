"""Known-region conditioning and partial-noise starts on the GPU: ``wd_known_blend`` against its host specification
(``tests/_known_ref.py``) bit for bit on guarded operands, its draws against the Philox specification, its argument checks, and
the three samplers around it - every step of a masked call replayed through the C-ABI, the identities a keep-mask must obey,
graph replay against eager launches, sharding, ``start``, one float64 trajectory and the driver's command line.

Bounds: equality of bits wherever two fp32 evaluations of the same expression are compared; ``TOL`` of
``tests/test_gpu_noise.py`` (derived there, relative to the radius) for a device draw against the float64 specification; 1e-4
max-norm relative for the float64 trajectory, the bar ``tests/test_gpu_ddim.py`` holds its own float64 trajectory to."""
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ddpm_oracle as D  # noqa: E402
from oracle import unet_oracle as U  # noqa: E402
from tests import _ddim_ref as R  # noqa: E402
from tests import _guard as G  # noqa: E402
from tests import _known_ref as K  # noqa: E402
from tests._common import SMALL, make_args, max_rel  # noqa: E402
from tests.test_gpu_noise import _check, _ddpm_z  # noqa: E402  (the bound of a device draw and the step kernel's own draw)
from worddiffusion_amd import Diffusion, UNetModel, UNetModelPhosc  # noqa: E402
from worddiffusion_amd import _native as N  # noqa: E402
from worddiffusion_amd.synthetic import fill_module_, synthetic_tensor  # noqa: E402

DEV = "cuda:0"
HW = (32, 64)
SHAPE = (4, 4, 8)  # the latent of HW
NPIX = 128
T = 8
CFG339 = dict(SMALL, num_classes=339)
BIG = (3, 4 * 2 ** 18)  # more float4s than the 2048 x 256 threads a launch is capped at: the second grid-stride pass starts at row 2
SAMPLERS = ["ddpm", "ddim", "dpmpp"]


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _i32(*v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def _blend(x, x0, mask, batch, n, sa, sb, t=None, k=None, tau=None, S=0, noise=None, seed=0, offset=0):
    return N.lib().wd_known_blend(_ptr(x), _ptr(x0), _ptr(mask), batch, n, _ptr(sa), _ptr(sb), _ptr(t), _ptr(k), _ptr(tau), S,
                                  _ptr(noise), seed, offset, _st())


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def tables():
    """sqrt(alpha_hat), sqrt(1 - alpha_hat) of a 12-step schedule, on the device and as the numpy arrays the specification reads."""
    sa, sb = Diffusion(noise_steps=12)._noise_tables(DEV)
    return sa, sb, sa.cpu().numpy(), sb.cpu().numpy()


def _mask_values(batch, n, g):
    """0, 1 and fractional values in every row (n = 4: one row holds 0, 1 and two fractions)."""
    m = torch.rand(batch, n, generator=g)
    pick = torch.randint(0, 3, (batch, n), generator=g)
    m = torch.where(pick == 0, torch.zeros(()), torch.where(pick == 1, torch.ones(()), m))
    m[:, 0], m[:, 1], m[:, 2] = 0.0, 1.0, 0.3
    return m


# ------------------------------------------------------------------------------------------------ 1. kernel against the specification
FORMS = {  # name -> (t, k, tau): the DDPM form at t = 7 and at t = 1 (p = 0), the table form at k = 0 and at k = S - 1 (p = 0)
    "ddpm": (7, None, None), "ddpm-last": (1, None, None), "table": (None, 0, [11, 8, 3]), "table-mid": (None, 1, [11, 8, 3]),
    "table-last": (None, 2, [11, 8, 3])}


# every form at the small shapes; past the grid cap one form that reads the noise and one that ends on p = 0
CASES = [(b, n, f) for b in (1, 3) for n in (4, 1024) for f in sorted(FORMS)] + [BIG + ("ddpm",), BIG + ("table-last",)]


@pytest.mark.parametrize("batch,n,form", CASES)
def test_kernel_bit_equal_to_the_specification(tables, batch, n, form):
    sa, sb, sa_np, sb_np = tables
    t, k, tau = FORMS[form]
    p = K.predecessor(t=t, k=k, tau=tau)
    assert p == {"ddpm": 6, "ddpm-last": 0, "table": 8, "table-mid": 3, "table-last": 0}[form]
    g = torch.Generator().manual_seed(batch * 7 + n)
    x, x0, z = (torch.randn(batch, n, generator=g) for _ in range(3))
    m = _mask_values(batch, n, g)
    bufs = {}
    for name, val in (("x", x), ("x0", x0), ("mask", m), ("noise", z)):
        buf, view = G.guarded_flat(batch * n, torch.float32, device=DEV)
        if not (name == "noise" and p == 0):  # at p == 0 the noise is not read: it stays the NaN pattern
            view.copy_(val.reshape(-1))
        bufs[name] = (buf, view)
    rc = _blend(bufs["x"][1], bufs["x0"][1], bufs["mask"][1], batch, n, sa, sb, t=None if t is None else _i32(t),
                k=None if k is None else _i32(k), tau=None if tau is None else _i32(*tau), S=len(tau or ()), noise=bufs["noise"][1])
    torch.cuda.synchronize()
    assert rc == N.WD_OK
    for name, (buf, view) in bufs.items():
        G.assert_untouched(buf, view, name)
    got = bufs["x"][1].reshape(batch, n)
    G.assert_finite(got, "x")
    for name, val in (("x0", x0), ("mask", m)):
        assert torch.equal(bufs[name][1].cpu().reshape(batch, n), val), f"{name} was written"
    want = K.blend(x.numpy(), x0.numpy(), m.numpy(), p, sa_np, sb_np, None if p == 0 else z.numpy())
    assert _same_bits(got, torch.from_numpy(want))
    # the three branches are live in this case: kept bits, replaced values, blended values
    keep0, keep1 = (m == 0), (m == 1)
    assert keep0.any() and keep1.any() and (~keep0 & ~keep1).any()
    assert torch.equal(got.cpu()[keep0], x[keep0]) and not torch.equal(got.cpu()[keep1], x[keep1])
    if p == 0:
        assert torch.equal(got.cpu()[keep1], x0[keep1])


@pytest.mark.parametrize("p", [1, 6, 10])
def test_full_mask_equals_noise_images(p):
    """m == 1 everywhere: what the blend leaves is ``Diffusion.noise_images(x0, p, eps=z)``, bit for bit."""
    diff = Diffusion(noise_steps=12, img_size=HW, args=make_args(device=DEV))
    sa, sb = diff._noise_tables(DEV)
    g = torch.Generator().manual_seed(p)
    x, x0, z = (torch.randn(3, *SHAPE, generator=g).to(DEV) for _ in range(3))
    ones = torch.ones(3, NPIX, device=DEV)
    want, _ = diff.noise_images(x0, torch.full((3,), p, dtype=torch.int64), eps=z)
    for kw in (dict(t=_i32(p + 1)), dict(k=_i32(0), tau=_i32(11, p), S=2)):
        got = x.clone()
        assert _blend(got, x0, ones, 3, NPIX, sa, sb, noise=z, **kw) == N.WD_OK
        torch.cuda.synchronize()
        assert _same_bits(got, want), kw


# ------------------------------------------------------------------------------------------------ 2. the kernel's own draws
def _known_z(batch, n, p, seed, offset, mask=None, table=False):
    """Tables sqrt_ah = 0, sqrt_1m_ah = 1, x0 = 0, m = 1: what the blend leaves in x is the z it drew at level p."""
    zeros, ones = torch.zeros(1000, device=DEV), torch.ones(1000, device=DEV)
    x = torch.full((batch, n), float("nan"), device=DEV)
    x0 = torch.zeros(batch, n, device=DEV)
    m = torch.ones(batch, n, device=DEV) if mask is None else mask
    kw = dict(k=_i32(0), tau=_i32(999, p), S=2) if table else dict(t=_i32(p + 1))
    N.check(_blend(x, x0, m, batch, n, zeros, ones, seed=seed, offset=offset, **kw), "wd_known_blend")
    torch.cuda.synchronize()
    return x


@pytest.mark.parametrize("p", [1, 2, 500, 998])
def test_draws_equal_the_philox_specification(p):
    seed, offset = 2 ** 32 + 77, 6
    ref = K.draw(3, 128, seed, offset, p, with_r=True)
    got = _known_z(3, 128, p, seed, offset)
    _check(got, ref, f"wd_known_blend p={p}")
    assert torch.equal(got, _known_z(3, 128, p, seed, offset, table=True))  # both forms of p: the same draw


def test_draws_past_the_grid_cap():
    batch, n = BIG
    _check(_known_z(batch, n, 500, 77, 6), K.draw(batch, n, 77, 6, 500, with_r=True), f"wd_known_blend {batch} x {n} p=500")


def test_every_key_word_of_the_draw_is_live():
    base = _known_z(3, 128, 5, 77, 6)
    assert torch.equal(base, _known_z(3, 128, 5, 77, 6))
    assert not torch.equal(base, _known_z(3, 128, 5, 78, 6))             # seed
    assert not torch.equal(base, _known_z(3, 128, 5, 2 ** 32 + 77, 6))   # its high word
    assert not torch.equal(base, _known_z(3, 128, 4, 77, 6))             # p
    assert not torch.equal(base[0], base[1]) and not torch.equal(base[:, :4], base[:, 4:8])  # row, element counter
    shifted = _known_z(3, 128, 5, 77, 7)                                 # sample_offset: rows 7, 8, 9
    assert torch.equal(shifted[:2], base[1:]) and not torch.equal(shifted[2], base[2])
    assert not torch.equal(base, _known_z(3, 128, 5, 77, 2 ** 32 + 6))   # high word of the row
    # a tag family of its own: not the step kernel's draw at t = p, not any wd_randn stream at the same key
    assert not torch.equal(base, _ddpm_z(3, 128, 5, 77, 6))
    for stream_id in (0, 1, 2, 3, 4):
        r = torch.empty(3, 128, device=DEV)
        N.check(N.lib().wd_randn(r.data_ptr(), 3, 128, 77, 6, stream_id, _st()), "wd_randn")
        torch.cuda.synchronize()
        assert not torch.equal(base, r), stream_id
    # the draw of a group of four does not depend on its mask: element 1 of every group kept alone sees the z of the full mask
    m = torch.zeros(3, 128, device=DEV)
    m[:, 1::4] = 1.0
    part = _known_z(3, 128, 5, 77, 6, mask=m)
    assert torch.equal(part[:, 1::4], base[:, 1::4]) and bool(torch.isnan(part[:, 0::4]).all())  # (x was NaN where m == 0: kept)


# ------------------------------------------------------------------------------------------------ 3. argument checks
def test_einval_launches_nothing(tables):
    sa, sb = tables[:2]
    batch, n = 2, 64
    g = torch.Generator().manual_seed(4)
    buf, x = G.guarded_flat(batch * n, torch.float32, device=DEV)
    before = torch.randn(batch * n, generator=g).to(DEV)
    x.copy_(before)
    x0, m, z = (torch.rand(batch * n + 4, generator=g).to(DEV) for _ in range(3))
    t, k, tau = _i32(7), _i32(0), _i32(11, 8, 3)
    good = dict(x=x, x0=x0[:-4], mask=m[:-4], batch=batch, n=n, sa=sa, sb=sb, t=t, k=None, tau=None, S=0, noise=z[:-4])
    off = lambda v: v[1:1 + batch * n]  # noqa: E731  (4 bytes past a 16-byte boundary)
    assert off(x0).data_ptr() % 16 == 4
    xbuf = torch.zeros(batch * n + 4, device=DEV)
    cases = [dict(x=None), dict(x0=None), dict(mask=None), dict(sa=None), dict(sb=None),
             dict(t=None),                                  # neither form of p
             dict(t=None, tau=tau, k=None, S=3),            # a table without its index
             dict(tau=tau, k=k, S=0), dict(tau=tau, k=k, S=-1),
             dict(n=62), dict(n=0), dict(batch=0),
             dict(x=off(xbuf)), dict(x0=off(x0)), dict(mask=off(m)), dict(noise=off(z))]
    for bad in cases:
        assert _blend(**dict(good, **bad)) == N.WD_EINVAL, sorted(bad)
    torch.cuda.synchronize()
    G.assert_untouched(buf, x, "x")
    assert torch.equal(x, before) and not xbuf.any()
    for form in (dict(), dict(tau=tau, k=k, S=3), dict(t=None, tau=tau, k=k, S=3), dict(noise=None)):  # and the call itself is good
        assert _blend(**dict(good, **form)) == N.WD_OK, sorted(form)
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


# ------------------------------------------------------------------------------------------------ 4. loop plumbing
@pytest.mark.parametrize("which,mode", [("ddpm", "fresh"), ("ddim", "fresh"), ("ddim", "fixed"), ("dpmpp", "fixed")])
def test_every_step_of_a_masked_call_replays_through_the_c_abi(setup, which, mode):
    """record[k], the recorded prediction, the sampler's own step kernel, then ``wd_known_blend`` with the expected p, tables, seed
    and offset: record[k + 1] (and at the end the returned latents), bit for bit."""
    m, diff, args, labels, words, known, cols, soft = setup
    lib = N.lib()
    n, seed, offset = 3, 41, 5
    eta = dict(eta=0.5) if (which, mode) == ("ddim", "fresh") else {}
    rec, preds = [], []
    out = _call(diff, which, m, n, words, labels, args, seed=seed, sample_offset=offset, known=known[:n], known_mask=soft,
                record=rec, record_pred=preds, **eta)
    st = diff.last_stats
    assert (st["known"], st["start"], st["known_noise"], st["graph"]) == (True, None, mode, False)
    tau = st.get("timesteps")
    S = len(tau) if tau else T - 1
    assert len(rec) == len(preds) == S == st["steps"]
    states = rec + [out]
    sa, sb = diff._noise_tables(DEV)
    x0 = known[:n].reshape(n, -1).to(DEV)
    mask = soft.expand(n, *SHAPE).reshape(n, -1).contiguous().to(DEV)
    keps = None
    if mode == "fixed":
        keps = torch.empty(n, NPIX, device=DEV)
        N.check(lib.wd_randn(keps.data_ptr(), n, NPIX, seed, offset, N.STREAM_KNOWN, _st()), "wd_randn")
    tau_dev = None if tau is None else _i32(*tau)
    if which == "ddpm":
        tabs = diff._step_tables(DEV)
    elif which == "ddim":
        tabs = diff._ddim_tables(tau, eta.get("eta", 0.0), DEV)
    else:
        tabs = diff._dpmpp_tables(tau, 2, DEV)
        x0_prev = torch.empty(n, NPIX, device=DEV)
    for k in range(S):
        x = states[k].clone()
        eps = preds[k][0]
        if which == "ddpm":
            t_dev, k_dev = _i32(T - 1 - k), None
            N.check(lib.wd_ddpm_step(x.data_ptr(), eps.data_ptr(), n, NPIX, *(c.data_ptr() for c in tabs), t_dev.data_ptr(), None,
                                     seed, offset, _st()), "wd_ddpm_step")
        elif which == "ddim":
            t_dev, k_dev = _i32(tau[k]), _i32(k)
            N.check(lib.wd_ddim_step(x.data_ptr(), eps.data_ptr(), None, 0.0, None, n, NPIX, *(c.data_ptr() for c in tabs),
                                     k_dev.data_ptr(), t_dev.data_ptr(), None, seed, offset, _st()), "wd_ddim_step")
        else:
            t_dev, k_dev = _i32(tau[k]), _i32(k)
            N.check(lib.wd_dpmpp_step(x.data_ptr(), eps.data_ptr(), None, 0.0, None, x0_prev.data_ptr(), n, NPIX,
                                      *(c.data_ptr() for c in tabs), k_dev.data_ptr(), _st()), "wd_dpmpp_step")
        torch.cuda.synchronize()
        assert not torch.equal(x, states[k + 1]), (k, "the blend changed nothing")
        N.check(_blend(x, x0, mask, n, NPIX, sa, sb, t=t_dev, k=k_dev, tau=tau_dev, S=len(tau or ()), noise=keps, seed=seed,
                       offset=offset), "wd_known_blend")
        torch.cuda.synchronize()
        assert _same_bits(x, states[k + 1]), (which, mode, k)
    assert torch.equal(out.reshape(n, *SHAPE)[..., :4].cpu(), known[:n][..., :4])


# ------------------------------------------------------------------------------------------------ 5. identities
@pytest.mark.parametrize("which", SAMPLERS)
def test_mask_identities(setup, which):
    m, diff, args, labels, words, known, cols, soft = setup
    n, kw = 3, dict(seed=17, sample_offset=2)
    plain = _call(diff, which, m, n, words, labels, args, **kw)
    assert (diff.last_stats["known"], diff.last_stats["start"], diff.last_stats["known_noise"]) == (False, None, None)
    assert torch.isfinite(plain).all() and float(plain.std()) > 0.05
    # all ones: the trajectory ends on the known latents themselves
    full = _call(diff, which, m, n, words, labels, args, known=known[:n], known_mask=torch.ones(SHAPE[1:]), **kw)
    assert _same_bits(full, known[:n])
    # all zeros: nothing is kept - the call without ``known``, bit for bit, in either noise mode
    for mode in ("fresh", "fixed"):
        none = _call(diff, which, m, n, words, labels, args, known=known[:n], known_mask=torch.zeros(SHAPE[1:]), known_noise=mode, **kw)
        assert diff.last_stats["known_noise"] == mode and _same_bits(none, plain), mode
    # a binary column mask: the kept columns ARE the known latents, the others are neither known nor the plain call's
    for mask in (cols, cols.expand(n, 1, *SHAPE[1:]), cols.expand(n, *SHAPE)):
        got = _call(diff, which, m, n, words, labels, args, known=known[:n], known_mask=mask, **kw)
        assert diff.last_stats["graph"] and diff.last_stats["known"]
        assert _same_bits(got[..., :4], known[:n][..., :4])
        assert torch.isfinite(got).all() and not torch.equal(got[..., 4:].cpu(), known[:n][..., 4:])
        assert not torch.equal(got[..., 4:], plain[..., 4:])  # the free region is drawn in the context of the kept one
    # a per-sample mask: row 0 kept whole, row 1 not at all, row 2 by columns
    per = torch.stack([torch.ones(1, *SHAPE[1:]), torch.zeros(1, *SHAPE[1:]), cols[None]])
    got = _call(diff, which, m, n, words, labels, args, known=known[:n], known_mask=per, **kw)
    assert _same_bits(got[0], known[0]) and _same_bits(got[1], plain[1]) and _same_bits(got[2, :, :, :4], known[2, :, :, :4])


def test_mix_rate_and_guided_steps_are_orthogonal():
    import random
    n, S = 3, 4
    labels = torch.tensor([4, 5, 6], dtype=torch.int64)
    g = torch.Generator().manual_seed(3)
    known = torch.randn(n, *SHAPE, generator=g)
    cols = torch.zeros(SHAPE[1:])
    cols[:, 5:] = 1.0
    diff = Diffusion(noise_steps=9, img_size=HW, args=make_args(device=DEV))
    # fixed pairs, one forward per step
    m = _model(UNetModelPhosc, CFG339, 9)
    kw = dict(steps=S, seed=21, mix_rate=torch.tensor([0.0, 0.5, 1.0]), style_pairs=(3, 7))
    a = diff.sampling_ddim(m, None, n, "text", labels, make_args(device=DEV), known=known, known_mask=cols, **kw)
    assert diff.last_stats["forwards_per_step"] == 1 and diff.last_stats["known_noise"] == "fixed"
    assert _same_bits(a[..., 5:], known[..., 5:]) and not torch.equal(a[..., :5].cpu(), known[..., :5])
    assert not torch.equal(a, diff.sampling_ddim(m, None, n, "text", labels, make_args(device=DEV), **kw))
    # reference mode with guidance: two forwards and the guided update, then the blend
    iargs = make_args(device=DEV, interpolation=True)
    mi = _model(UNetModelPhosc, CFG339, 9, interpolation=True)
    for call, extra in ((diff.sampling, {}), (diff.sampling_ddim, dict(steps=S)), (diff.sampling_dpmpp, dict(steps=S))):
        random.seed(31)
        b = call(mi, None, n, "text", labels, iargs, seed=21, mix_rate=0.37, cfg_scale=3, known=known, known_mask=cols, **extra)
        assert diff.last_stats["forwards_per_step"] == 2 and diff.last_stats["known"]
        assert _same_bits(b[..., 5:], known[..., 5:]) and torch.isfinite(b).all()


# ------------------------------------------------------------------------------------------------ 6. graph == eager
@pytest.mark.parametrize("which", SAMPLERS)
def test_graph_replay_equals_eager_with_a_mask_and_with_start(setup, which):
    m, diff, args, labels, words, known, cols, soft = setup
    n = 3
    for kw in (dict(known_mask=soft), dict(known_mask=soft, start=5), dict(start=5), dict(known_mask=soft, known_noise="fresh"),
               dict(known_mask=cols, start=6, known_noise="fixed")):
        outs = []
        for use_graph in (True, False):
            outs.append(_call(diff, which, m, n, words, labels, args, seed=23, sample_offset=1, known=known[:n], use_graph=use_graph, **kw))
            assert diff.last_stats["graph"] == use_graph
        assert _same_bits(outs[0], outs[1]), kw
        assert torch.isfinite(outs[0]).all()
        if "known_mask" in kw:
            assert _same_bits(outs[0][..., :4], known[:n][..., :4])


# ------------------------------------------------------------------------------------------------ 7. sharding, determinism
@pytest.mark.parametrize("which", SAMPLERS)
def test_fresh_mode_is_keyed_by_the_global_row(setup, which):
    m, diff, args, labels, words, known, cols, soft = setup
    eta = dict(eta=0.5) if which == "ddim" else {}
    kw = dict(seed=29, known_mask=soft, known_noise="fresh", **eta)
    whole = _call(diff, which, m, 4, words, labels, args, sample_offset=0, known=known, **kw)
    assert diff.last_stats["known_noise"] == "fresh"
    lo = _call(diff, which, m, 2, words, labels, args, sample_offset=0, known=known[:2], **kw)
    hi = _call(diff, which, m, 2, words[2:], labels[2:], args, sample_offset=2, known=known[2:], **kw)
    assert _same_bits(whole[:2], lo) and _same_bits(whole[2:], hi)
    assert not torch.equal(whole[..., 5:], _call(diff, which, m, 4, words, labels, args, sample_offset=0, known=known,
                                                 **dict(kw, seed=30))[..., 5:])
    # ... and so is the fixed eps, with ``start`` too
    kw = dict(seed=29, known_mask=soft, known_noise="fixed", start=5, **eta)
    whole = _call(diff, which, m, 4, words, labels, args, sample_offset=0, known=known, **kw)
    hi = _call(diff, which, m, 2, words[2:], labels[2:], args, sample_offset=2, known=known[2:], **kw)
    assert _same_bits(whole[2:], hi)


def test_eta0_ddim_with_the_fixed_eps_is_reproducible_from_the_seed(setup):
    m, diff, args, labels, words, known, cols, soft = setup
    kw = dict(known=known[:3], known_mask=soft)
    a = _call(diff, "ddim", m, 3, words, labels, args, seed=7, **kw)
    assert diff.last_stats["known_noise"] == "fixed" and diff.last_stats["eta"] == 0.0  # what "auto" means here
    assert _same_bits(a, _call(diff, "ddim", m, 3, words, labels, args, seed=7, **kw))
    assert _same_bits(a, _call(diff, "ddim", m, 3, words, labels, args, seed=7, known_noise="fixed", **kw))
    assert not torch.equal(a, _call(diff, "ddim", m, 3, words, labels, args, seed=8, **kw))
    # given x_T, the seed reaches the result through the fixed eps alone; given both, nothing is drawn
    X = torch.randn(3, *SHAPE, generator=torch.Generator().manual_seed(2))
    b = _call(diff, "ddim", m, 3, words, labels, args, seed=7, x_T=X, **kw)
    assert not torch.equal(b[..., 4:], _call(diff, "ddim", m, 3, words, labels, args, seed=8, x_T=X, **kw)[..., 4:])
    E = torch.randn(3, *SHAPE, generator=torch.Generator().manual_seed(3))
    c = _call(diff, "ddim", m, 3, words, labels, args, seed=7, x_T=X, known_noise=E, **kw)
    assert _same_bits(c, _call(diff, "ddim", m, 3, words, labels, args, seed=8, x_T=X, known_noise=E, **kw))
    # the deterministic samplers draw per step only when asked to
    d = _call(diff, "dpmpp", m, 3, words, labels, args, seed=7, x_T=X, **kw)
    assert diff.last_stats["known_noise"] == "fixed"
    e = _call(diff, "dpmpp", m, 3, words, labels, args, seed=7, x_T=X, known_noise="fresh", **kw)
    assert diff.last_stats["known_noise"] == "fresh" and not torch.equal(d[..., 4:], e[..., 4:])
    _call(diff, "ddpm", m, 3, words, labels, args, seed=7, **kw)
    assert diff.last_stats["known_noise"] == "fresh"


# ------------------------------------------------------------------------------------------------ 8. start
@pytest.mark.parametrize("which,start,level,visited", [("ddpm", 5, 5, None), ("ddpm", 1, 1, None), ("ddpm", 7, 7, None),
                                                       ("ddim", 6, 5, [5, 3, 1]), ("ddim", 7, 7, [7, 5, 3, 1]), ("ddim", 1, 1, [1]),
                                                       ("dpmpp", 4, 3, [3, 1]), ("dpmpp", 5, 5, [5, 3, 1])])
def test_start_noises_the_known_latents_and_visits_the_retained_steps(setup, which, start, level, visited):
    m, diff, args, labels, words, known, cols, soft = setup
    n, seed, offset = 3, 13, 4
    rec = []
    out = _call(diff, which, m, n, words, labels, args, seed=seed, sample_offset=offset, known=known[:n], start=start, record=rec)
    st = diff.last_stats
    steps = level if visited is None else len(visited)
    assert (st["known"], st["start"], st["steps"], st["model_calls"]) == (True, level, steps, steps) and len(rec) == steps
    assert st.get("timesteps") == visited
    assert st["known_noise"] == ("fresh" if which == "ddpm" else "fixed")
    eps = torch.empty(n, *SHAPE, device=DEV)
    N.check(N.lib().wd_randn(eps.data_ptr(), n, NPIX, seed, offset, N.STREAM_KNOWN, _st()), "wd_randn")
    _check(eps, K.fixed_eps(n, NPIX, seed, offset, with_r=True), "the fixed eps")
    want, _ = diff.noise_images(known[:n].to(DEV), torch.full((n,), level, dtype=torch.int64), eps=eps)
    assert _same_bits(rec[0], want)
    assert torch.isfinite(out).all() and not torch.equal(out.cpu(), known[:n])
    # the rest of the trajectory is the sampler's own from that state: the same timesteps from x_T = record[0]
    if which != "ddpm":
        again = _call(diff, which, m, n, words, labels, args, seed=seed, sample_offset=offset, x_T=rec[0], timesteps=visited)
        assert diff.last_stats["timesteps"] == visited and _same_bits(again, out)
    elif level == T - 1:
        assert _same_bits(_call(diff, which, m, n, words, labels, args, seed=seed, sample_offset=offset, x_T=rec[0]), out)
    # a given eps takes the place of the drawn one
    E = torch.randn(n, *SHAPE, generator=torch.Generator().manual_seed(9))
    rec2 = []
    _call(diff, which, m, n, words, labels, args, seed=seed, known=known[:n], start=start, known_noise=E, record=rec2)
    want2, _ = diff.noise_images(known[:n].to(DEV), torch.full((n,), level, dtype=torch.int64), eps=E.to(DEV))
    assert _same_bits(rec2[0], want2) and diff.last_stats["known_noise"] == "fixed"


def test_sampler_errors_and_model_state(setup):
    m, diff, args, labels, words, known, cols, soft = setup
    with pytest.raises(ValueError):  # C of ``known`` against the model's latent: settled where the plan is known
        diff.sampling_ddim(m, None, 3, words[:3], labels[:3], args, steps=4, known=torch.zeros(3, 2, 4, 8), known_mask=cols)
    with pytest.raises(ValueError):
        diff.sampling_ddim(m, None, 3, words[:3], labels[:3], args, timesteps=[7, 5], known=known[:3], start=4)
    m.eval()
    out = diff.sampling_dpmpp(m, None, 3, words[:3], labels[:3], args, steps=3, known=known[:3], known_mask=cols, start=6)
    assert m.training and out.shape == (3, *SHAPE)  # eval mode for the loop, TRAIN mode afterwards, as without ``known``
    m.eval()


# ------------------------------------------------------------------------------------------------ 9. one float64 trajectory
def test_masked_ddim_trajectory_matches_float64_oracle():
    """DDIM, eta = 0, 4 visited steps, a given ``known_noise``, the first half of the columns kept: every state against the CPU
    oracle UNet with the update (``tests/_ddim_ref.py``) and the blend in float64, to the bar of
    ``test_gpu_ddim.test_ddim_trajectory_matches_float64_oracle``."""
    S, n, seed = 4, 3, 9
    args = make_args(device=DEV)
    m = _model(UNetModel, SMALL, seed)
    diff = Diffusion(noise_steps=T, img_size=HW, args=args)
    tau = diff.ddim_timesteps(S)
    assert tau == [7, 5, 3, 1]
    g = torch.Generator().manual_seed(3)
    x_T, known, E = (torch.randn(n, *SHAPE, generator=g) for _ in range(3))
    mask = torch.zeros(SHAPE[1:])
    mask[:, :4] = 1.0
    labels = torch.tensor([1, 7, 10], dtype=torch.int64)
    word = "Moving"
    rec = []
    out = diff.sampling_ddim(m, None, n, word, labels, args, steps=S, eta=0.0, x_T=x_T, known=known, known_mask=mask, known_noise=E,
                             record=rec)
    assert diff.last_stats["model_calls"] == S and diff.last_stats["known_noise"] == "fixed"
    sd = {k: torch.from_numpy(synthetic_tensor(k, s, seed)).double() for k, s in U.state_dict_shapes(SMALL, "base")}
    orc = U.UNetOracle(SMALL, sd, "base", False)
    ctx = torch.tensor([D.label_padding(word)] * n, dtype=torch.int64)
    ah = R.alpha_hat64(T)
    c = R.tables(T, tau, 0.0)
    x, x0, z, mk = x_T.double(), known.double(), E.double(), mask.double()
    ref = []
    with torch.no_grad():
        for k, t in enumerate(tau):
            ref.append(x.clone())
            eps = orc(x, torch.full((n,), t, dtype=torch.int64), ctx, labels, None).double()
            x = R.step(c, k, x, eps)
            p = K.predecessor(k=k, tau=tau)
            kv = x0 if p == 0 else torch.sqrt(ah[p]) * x0 + torch.sqrt(1 - ah[p]) * z
            x = x + mk * (kv - x)
    xs = torch.stack([r.cpu() for r in rec] + [out.cpu()])
    ref_xs = torch.stack(ref + [x])
    assert xs.shape == ref_xs.shape == (S + 1, n, *SHAPE)
    errs = [max_rel(xs[k], ref_xs[k]) for k in range(S + 1)]
    print(f"masked ddim trajectory: max_rel per state {['%.2e' % e for e in errs]}")
    assert max(errs) < 1e-4
    assert torch.equal(out[..., :4].cpu(), known[..., :4])


# ------------------------------------------------------------------------------------------------ 10. driver
def test_driver_command_line_from_init_latents(golden_dir, tmp_path, monkeypatch):
    from worddiffusion_amd import driver
    from worddiffusion_amd.latents import LatentCache, save_latent_cache
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    gt = tmp_path / "gt.txt"
    lines = [ln for ln in open(os.path.join(golden_dir, "gt_samples.txt")).read().splitlines() if ln.strip()]
    gt.write_text("\n".join([ln for ln in lines if not ln.startswith("#")][:3]) + "\n")
    rows = driver.read_gt(str(gt))
    assert len(rows) == 3 and len({r[1] for r in rows}) == 3
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
            "--seed", "5", "--init_latents", cache, "--keep_cols", "0:12", "--start", "8"]
    driver.main(base + ["--sampler", "ddim", "--ddim_steps", "4"])
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
                                 known=kn, known_mask=mask, start=8).cpu()
        assert diff.last_stats["timesteps"] == [7, 4, 1] and diff.last_stats["start"] == 7
        for (_, image, _), r, k0 in zip(chunk, ref, kn):
            got = np.load(out / "images" / f"{image}.npy")
            assert np.array_equal(got, r.numpy()), image
            assert np.array_equal(got[:, :, :12], k0.numpy()[:, :, :12]) and not np.array_equal(got[:, :, 12:], k0.numpy()[:, :, 12:])
    # the other two samplers take the same flags; the step-skipping sampler does not
    for extra in (["--sampler", "dpmpp", "--dpmpp_steps", "3"], []):
        out2 = tmp_path / ("out_" + (extra[1] if extra else "ddpm"))
        driver.main([str(out2) if a == str(out) else a for a in base] + extra)
        for _, image, _ in rows:
            got = np.load(out2 / "images" / f"{image}.npy")
            assert np.array_equal(got[:, :, :12], latents[image + ".png"].numpy()[:, :, :12]) and np.isfinite(got).all()
    with pytest.raises(SystemExit):
        driver.main(base + ["--skip_steps", "1"])
    # a row that the cache does not hold is an error that names it
    save_latent_cache(str(tmp_path / "short.npz"), {k: v for k, v in list(latents.items())[:2]})
    with pytest.raises(KeyError, match=re.escape(rows[2][1])):
        driver.regenerate(m, diff, rows, wr, args, known=LatentCache(str(tmp_path / "short.npz")), keep_cols=(0, 12), rank=0, world=1)
