"""The small kernels at the two ends of every forward, sampling step and training step (csrc/wd_misc.hip) behind guard bands and
past the grid cap, against tests/_edge_ref.py (held to the oracle by tests/test_edge_ref_host.py).

Every operand is a window of a wider buffer filled with a NaN pattern (tests/_guard.py): a store outside the window changes the
pattern, a read outside it brings a NaN into the result.  Every kernel with a grid-stride loop runs all cases of its table: one
with more work items than ``grid_for`` launches threads for (a ragged second pass that begins inside the last sample) and two
inside one block.

Bit for bit (``torch.equal``; planes as int16): the DDPM updates, noise_images, the EMA, the layout changes, im2col, the token
embedding, the timestep advance.  Device draws: ``tests/_philox_ref.py`` evaluates log, sqrt, sin and cos in float64, so no host
value carries the bits of a device draw.  A launch's draws are therefore held (a) to the Philox reference under the key
(seed, sample_offset + b, tag, e4) within test_gpu_noise's DRAW_TOL * radius, every element - a wrong index moves a draw by
O(1) - and (b) bit for bit to single-sample launches of the same rows, which stay inside the first pass; the update that adds
them is then compared bit for bit with the specification fed those draws.
|got - ref| <= 2^-16 |ref| + 1e-6 against float64 for wd_emb_combine (two bf16 roundings; SiLU through expf), 2e-5 absolute for
wd_timestep_embedding.  The refusal tests at the end pass one bad argument at a time; those calls return before any launch."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _edge_ref as E  # noqa: E402
from tests import _guard as G  # noqa: E402
from tests import _philox_ref as P  # noqa: E402
from worddiffusion_amd import _native as N  # noqa: E402

DEV = "cuda:0"
SEED, OFFSET = 77, 6


def _st():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _flat(x):
    """x as a guarded contiguous run on the device: (buf, view 1-D)."""
    buf, view = G.guarded_flat(x.numel(), x.dtype, device=DEV)
    view.copy_(x.reshape(-1))
    return buf, view


def _i64(values):
    """An int64 vector as a guarded run of int32 pairs (tests/_guard.py has no int64 pattern): (buf int32, view int64)."""
    v = torch.as_tensor(values, dtype=torch.int64).reshape(-1)
    buf, view = G.guarded_flat(2 * v.numel(), torch.int32, device=DEV)
    v64 = view.view(torch.int64)
    v64.copy_(v)
    return buf, v64


def _i64_untouched(buf, view64, name):
    G.assert_untouched(buf, (0, 1, view64.storage_offset() * 2 - buf.storage_offset(), 2 * view64.numel()), name)


def _rows(x, ld=None, col0=0):
    """The 2-D tensor x as a window with guard rows above and below (and to the right when ld > cols)."""
    return G.pitched(x, x.shape[1] if ld is None else ld, col0, device=DEV)


def _planes_out(rows, cols, ld):
    return G.guarded(rows, cols, ld, 0, torch.bfloat16, device=DEV, planes=2)


def _bits(p):
    return p.detach().cpu().contiguous().view(torch.int16)


def _value(p):
    p = p.detach().cpu()
    return p[0].float().double() + p[1].float().double()


def _untouched(pairs):
    for name, (buf, view) in pairs.items():
        G.assert_untouched(buf, view, name)


def _same(inputs):
    """Inputs the kernel must not write: the windows still hold what was put there."""
    for name, ((buf, view), want) in inputs.items():
        G.assert_untouched(buf, view, name)
        assert torch.equal(view.detach().cpu().reshape(-1), want.reshape(-1)), f"{name}: an input was written"


def _hi_only(launch, rows, cols, ld, both):
    """The launch with out_lo == NULL into fresh poisoned planes: its hi plane is the two-plane call's bit for bit, and the lo
    plane, passed nowhere, keeps the pattern in every element."""
    buf, view = _planes_out(rows, cols, ld)
    launch(view[0].data_ptr(), None)
    torch.cuda.synchronize()
    G.assert_untouched(buf[0], view[0], "hi plane (out_lo == NULL)")
    G.assert_untouched(buf[1], (0, 0, 0, 0), "lo plane (out_lo == NULL)")
    assert torch.equal(_bits(view[0]), _bits(both[0]))


def _tables():
    return [_flat(t) for t in E.step_tables(1000)]


def _t_dev(t):
    return _flat(torch.tensor([t], dtype=torch.int32))


# ------------------------------------------------------------------------------------------------ the DDPM update
def _ddpm(x, eps, c, tabs, t_dev, noise, seed=SEED, offset=OFFSET):
    N.check(N.lib().wd_ddpm_step(x.data_ptr(), eps.data_ptr(), c["batch"], c["n"], tabs[0].data_ptr(), tabs[1].data_ptr(),
                                 tabs[2].data_ptr(), t_dev.data_ptr(), None if noise is None else noise.data_ptr(), seed, offset,
                                 _st()), "wd_ddpm_step")
    torch.cuda.synchronize()


def _identity_tables():
    """ca = 1, cb = 0, cs = 1: on x = eps = 0 an update leaves exactly the z it drew."""
    ones, zeros = torch.ones(1000), torch.zeros(1000)
    return _flat(ones), _flat(zeros), _flat(ones)


@pytest.mark.parametrize("c", **E.params("wd_ddpm_step"))
def test_ddpm_step_given_noise(c):
    B, n = c["batch"], c["n"]
    x0, eps0, z0 = (E.rand((B, n), 100 + i) for i in range(3))
    tabs = _tables()
    for t in (999, 2):
        x, eps, z, td = _flat(x0), _flat(eps0), _flat(z0), _t_dev(t)
        _ddpm(x[1], eps[1], c, [v for _, v in tabs], td[1], z[1])
        G.assert_untouched(*x, "x")
        G.assert_finite(x[1], "x")
        assert torch.equal(x[1].cpu().reshape(B, n), E.ddpm_update(x0, eps0, *E.step_tables(1000)[:3], t, z0)), t
        _same({"eps": (eps, eps0), "noise": (z, z0), "t_dev": (td, torch.tensor([t], dtype=torch.int32))})
    for name, tv, want in zip(("ca", "cb", "cs"), tabs, E.step_tables(1000)):
        _same({name: (tv, want)})


@pytest.mark.parametrize("c", **E.params("wd_ddpm_step"))
def test_ddpm_step_device_draws(c):
    B, n, t = c["batch"], c["n"], 500
    ident = _identity_tables()
    zx, ze, td = _flat(torch.zeros(B, n)), _flat(torch.zeros(B, n)), _t_dev(t)
    _ddpm(zx[1], ze[1], c, [v for _, v in ident], td[1], None)
    G.assert_untouched(*zx, "x (identity tables)")
    z_dev = zx[1].cpu().reshape(B, n)
    worst = E.draws_within(z_dev, E.draws(B, n, SEED, OFFSET, t))
    print(f"wd_ddpm_step draws {E.case_id(c)}: err/tol {worst:.4f}")
    assert worst <= 1.0
    for b in {0, B - 1}:  # the rows as single-sample launches (inside the first pass) draw the same bits
        one = _flat(torch.zeros(1, n))
        _ddpm(one[1], ze[1][:n], dict(batch=1, n=n), [v for _, v in ident], td[1], None, offset=OFFSET + b)
        assert torch.equal(one[1].cpu(), z_dev[b]), b
    x0, eps0 = E.rand((B, n), 110), E.rand((B, n), 111)
    tabs = _tables()
    x, eps = _flat(x0), _flat(eps0)
    _ddpm(x[1], eps[1], c, [v for _, v in tabs], td[1], None)
    G.assert_untouched(*x, "x")
    assert torch.equal(x[1].cpu().reshape(B, n), E.ddpm_update(x0, eps0, *E.step_tables(1000)[:3], t, z_dev))
    _same({"eps": (eps, eps0), "t_dev": (td, torch.tensor([t], dtype=torch.int32))})


@pytest.mark.parametrize("t", [1, 0])
@pytest.mark.parametrize("c", **E.params("wd_ddpm_step"))
def test_ddpm_step_last_steps_add_nothing_and_ignore_the_seed(c, t):
    B, n = c["batch"], c["n"]
    x0, eps0 = E.rand((B, n), 120), E.rand((B, n), 121)
    tabs = [v for _, v in _tables()]
    ref = E.ddpm_update(x0, eps0, *E.step_tables(1000)[:3], t, None)
    got = []
    for seed in (1, 2 ** 40 + 5):
        x, eps, td = _flat(x0), _flat(eps0), _t_dev(t)
        _ddpm(x[1], eps[1], c, tabs, td[1], None, seed=seed)
        G.assert_untouched(*x, "x")
        got.append(x[1].cpu().reshape(B, n))
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], ref)


def _cfg(x, first, second, scale, eps_out, c, tabs, t_dev, noise):
    N.check(N.lib().wd_ddpm_step_cfg(x.data_ptr(), first.data_ptr(), second.data_ptr(), scale,
                                     None if eps_out is None else eps_out.data_ptr(), c["batch"], c["n"], tabs[0].data_ptr(),
                                     tabs[1].data_ptr(), tabs[2].data_ptr(), t_dev.data_ptr(),
                                     None if noise is None else noise.data_ptr(), SEED, OFFSET, _st()), "wd_ddpm_step_cfg")
    torch.cuda.synchronize()


@pytest.mark.parametrize("given_noise", [False, True])
@pytest.mark.parametrize("scale", E.GUIDE_SCALES)
@pytest.mark.parametrize("c", **E.params("wd_ddpm_step_cfg"))
def test_ddpm_step_cfg(c, scale, given_noise):
    B, n, t = c["batch"], c["n"], 17
    x0, f0, s0, z0 = (E.rand((B, n), 130 + i) for i in range(4))
    td = _t_dev(t)
    if given_noise:
        z, z_val = _flat(z0), z0
    else:  # the kernel's own draws, through identity tables on zeros: eps = lerp(0, 0) = 0
        ident = _identity_tables()
        zx, zf, zs = (_flat(torch.zeros(B, n)) for _ in range(3))
        _cfg(zx[1], zf[1], zs[1], scale, None, c, [v for _, v in ident], td[1], None)
        G.assert_untouched(*zx, "x (identity tables)")
        z, z_val = None, zx[1].cpu().reshape(B, n)
        worst = E.draws_within(z_val, E.draws(B, n, SEED, OFFSET, t))
        print(f"wd_ddpm_step_cfg draws {E.case_id(c)}: err/tol {worst:.4f}")
        assert worst <= 1.0
    tabs = _tables()
    x, first, second = _flat(x0), _flat(f0), _flat(s0)
    eo = G.guarded_flat(B * n, torch.float32, device=DEV)
    _cfg(x[1], first[1], second[1], scale, eo[1], c, [v for _, v in tabs], td[1], None if z is None else z[1])
    _untouched({"x": x, "eps_out": eo})
    G.assert_finite(eo[1], "eps_out")
    eps = E.guided_eps(f0, s0, scale)
    assert torch.equal(eo[1].cpu().reshape(B, n), eps)
    assert torch.equal(x[1].cpu().reshape(B, n), E.ddpm_update(x0, eps, *E.step_tables(1000)[:3], t, z_val))
    _same({"first": (first, f0), "second": (second, s0), "t_dev": (td, torch.tensor([t], dtype=torch.int32))})
    if z is not None:
        _same({"noise": (z, z0)})
    x2 = _flat(x0)  # eps_out is optional
    _cfg(x2[1], first[1], second[1], scale, None, c, [v for _, v in tabs], td[1], None if z is None else z[1])
    G.assert_untouched(*x2, "x")
    assert torch.equal(x2[1], x[1])


# ------------------------------------------------------------------------------------------------ wd_randn
def _randn(out, batch, n, offset, stream_id=0):
    N.check(N.lib().wd_randn(out.data_ptr(), batch, n, 1234, offset, stream_id, _st()), "wd_randn")
    torch.cuda.synchronize()


@pytest.mark.parametrize("c", **E.params("wd_randn"))
def test_randn(c):
    B, n = c["batch"], c["n"]
    out = G.guarded_flat(B * n, torch.float32, device=DEV)
    _randn(out[1], B, n, 5)
    G.assert_untouched(*out, "out")
    G.assert_finite(out[1], "out")
    got = out[1].cpu().reshape(B, n)
    worst = E.draws_within(got, E.draws(B, n, 1234, 5, P.STREAM | 0))
    print(f"wd_randn {E.case_id(c)}: err/tol {worst:.4f}")
    assert worst <= 1.0
    for b in range(B):  # every row as a launch of its own, inside the first pass
        assert n // 4 <= E.GRID_CAP_ITEMS
        one = G.guarded_flat(n, torch.float32, device=DEV)
        _randn(one[1], 1, n, 5 + b)
        G.assert_untouched(*one, "out (one row)")
        assert torch.equal(one[1].cpu(), got[b]), b


# ------------------------------------------------------------------------------------------------ noise_images, EMA
@pytest.mark.parametrize("c", **E.params("wd_noise_images"))
def test_noise_images(c):
    B, n = c["batch"], c["n"]
    x0, eps0 = E.rand((B, n), 140), E.rand((B, n), 141)
    t0 = torch.tensor([999, 0, 300][:B], dtype=torch.int64)  # both ends of the tables
    _, _, _, sa0, sb0 = E.step_tables(1000)
    x, eps, t, sa, sb = _flat(x0), _flat(eps0), _i64(t0), _flat(sa0), _flat(sb0)
    out = G.guarded_flat(B * n, torch.float32, device=DEV)
    N.check(N.lib().wd_noise_images(x[1].data_ptr(), eps[1].data_ptr(), t[1].data_ptr(), sa[1].data_ptr(), sb[1].data_ptr(), B, n,
                                    out[1].data_ptr(), _st()), "wd_noise_images")
    torch.cuda.synchronize()
    G.assert_untouched(*out, "out")
    G.assert_finite(out[1], "out")
    assert torch.equal(out[1].cpu().reshape(B, n), E.noise_images(x0, eps0, t0, sa0, sb0))
    _same({"x": (x, x0), "eps": (eps, eps0), "sqrt_ah": (sa, sa0), "sqrt_1m_ah": (sb, sb0)})
    _i64_untouched(*t, "t")
    assert torch.equal(t[1].cpu(), t0)


@pytest.mark.parametrize("beta", E.EMA_BETAS)
@pytest.mark.parametrize("c", **E.params("wd_ema_update"))
def test_ema_update(c, beta):
    n = c["n"]
    e0, p0 = E.rand((n,), 150), E.rand((n,), 151)
    ema, p = _flat(e0), _flat(p0)
    N.check(N.lib().wd_ema_update(ema[1].data_ptr(), p[1].data_ptr(), n, beta, _st()), "wd_ema_update")
    torch.cuda.synchronize()
    G.assert_untouched(*ema, "ema")
    G.assert_finite(ema[1], "ema")
    assert torch.equal(ema[1].cpu(), E.ema_update(e0, p0, beta))
    _same({"p": (p, p0)})


# ------------------------------------------------------------------------------------------------ layouts, im2col
@pytest.mark.parametrize("c", **E.params("wd_nchw_to_tokens"))
def test_nchw_to_tokens_into_a_wider_buffer(c):
    B, ch, hw, ld = c["batch"], c["c"], c["hw"], c["ld"]
    x0 = E.rand((B, ch, hw), 160)
    x = _flat(x0)
    out = G.guarded(B * hw, ch, ld, 0, torch.float32, device=DEV)
    N.check(N.lib().wd_nchw_to_tokens(x[1].data_ptr(), B, ch, hw, out[1].data_ptr(), ld, _st()), "wd_nchw_to_tokens")
    torch.cuda.synchronize()
    G.assert_untouched(*out, "out")
    G.assert_finite(out[1], "out")
    assert torch.equal(out[1].cpu(), E.nchw_to_tokens(x0))
    _same({"x": (x, x0)})


@pytest.mark.parametrize("c", **E.params("wd_tokens_to_nchw"))
def test_tokens_to_nchw_from_a_wider_buffer(c):
    B, ch, hw, ld = c["batch"], c["c"], c["hw"], c["ld"]
    tok0 = E.rand((B * hw, ch), 161)
    tok = _rows(tok0, ld)
    out = G.guarded_flat(B * ch * hw, torch.float32, device=DEV)
    N.check(N.lib().wd_tokens_to_nchw(tok[1].data_ptr(), ld, B, ch, hw, out[1].data_ptr(), _st()), "wd_tokens_to_nchw")
    torch.cuda.synchronize()
    G.assert_untouched(*out, "out")
    G.assert_finite(out[1], "out")
    assert torch.equal(out[1].cpu().reshape(B, ch, hw), E.tokens_to_nchw(tok0, B))
    G.assert_untouched(*tok, "x")
    assert torch.equal(tok[1].cpu(), tok0)


@pytest.mark.parametrize("c", **E.params("wd_im2col3x3"))
def test_im2col3x3(c):
    B, cin, h, w, kpad = c["batch"], c["cin"], c["h"], c["w"], c["kpad"]
    x0 = E.rand((B, cin, h, w), 170)
    x = _flat(x0)
    rows = B * h * w
    buf, view = _planes_out(rows, kpad, kpad)

    def launch(hi, lo):
        N.check(N.lib().wd_im2col3x3(x[1].data_ptr(), B, cin, h, w, hi, lo, kpad, _st()), "wd_im2col3x3")

    launch(view[0].data_ptr(), view[1].data_ptr())
    torch.cuda.synchronize()
    G.assert_untouched(buf, view, "planes")
    G.assert_finite(view, "planes")
    assert torch.equal(_bits(view), _bits(G.split_planes(E.im2col3x3(x0, kpad))))
    _same({"x": (x, x0)})
    _hi_only(launch, rows, kpad, kpad, view)


# ------------------------------------------------------------------------------------------------ the token embedding
def _embed_operands(c, seed):
    vocab, cc, seq = c["vocab"], c["c"], c["seq_len"]
    return E.rand((vocab, cc), seed), E.rand((seq, cc), seed + 1)


def _embed(ids_ptr, i64, rows, seq, table, pe, hi, lo, ld):
    N.check(N.lib().wd_embed_tokens(ids_ptr, i64, rows, seq, table.data_ptr(), table.shape[0], table.shape[1],
                                    None if pe is None else pe.data_ptr(), hi, lo, ld, _st()), "wd_embed_tokens")


@pytest.mark.parametrize("use_pe", [True, False])
@pytest.mark.parametrize("i64", [1, 0])
@pytest.mark.parametrize("c", **E.params("wd_embed_tokens"))
def test_embed_tokens(c, i64, use_pe):
    rows, seq, vocab, cc = c["rows"], c["seq_len"], c["vocab"], c["c"]
    table0, pe0 = _embed_operands(c, 180)
    ids0 = torch.randint(0, vocab, (rows,), generator=torch.Generator().manual_seed(182))
    ids0[0], ids0[-1] = vocab - 1, 0
    table, pe = _rows(table0), _rows(pe0)
    ids = _i64(ids0) if i64 else _flat(ids0.to(torch.int32))
    ld = cc + 8
    buf, view = _planes_out(rows, cc, ld)

    def launch(hi, lo):
        _embed(ids[1].data_ptr(), i64, rows, seq, table[1], pe[1] if use_pe else None, hi, lo, ld)

    launch(view[0].data_ptr(), view[1].data_ptr())
    torch.cuda.synchronize()
    G.assert_untouched(buf, view, "planes")
    G.assert_finite(view, "planes")
    assert torch.equal(_bits(view), _bits(G.split_planes(E.embed_tokens(ids0, table0, pe0 if use_pe else None, seq))))
    _untouched({"table": table, "pe": pe})
    assert torch.equal(table[1].cpu(), table0) and torch.equal(pe[1].cpu(), pe0)
    if i64:
        _i64_untouched(*ids, "ids")
    else:
        G.assert_untouched(*ids, "ids")
    _hi_only(launch, rows, cc, ld, view)


@pytest.mark.parametrize("i64", [1, 0])
def test_embed_tokens_clamps_ids_outside_the_vocabulary(i64):
    c = dict(rows=6, seq_len=3, vocab=53, c=64)
    table0, pe0 = _embed_operands(c, 185)
    ids0 = torch.tensor([-3, 53 + 7, 0, 52, -2 ** 31, 2 ** 31 - 1])
    table, pe = _rows(table0), _rows(pe0)
    ids = _i64(ids0) if i64 else _flat(ids0.to(torch.int32))
    buf, view = _planes_out(6, 64, 72)
    _embed(ids[1].data_ptr(), i64, 6, 3, table[1], pe[1], view[0].data_ptr(), view[1].data_ptr(), 72)
    torch.cuda.synchronize()
    G.assert_untouched(buf, view, "planes")
    G.assert_finite(view, "planes")
    want = table0[[0, 52, 0, 52, 0, 52]] + pe0[[0, 1, 2, 0, 1, 2]]
    assert torch.equal(_bits(view), _bits(G.split_planes(want)))
    assert torch.equal(_bits(view), _bits(G.split_planes(E.embed_tokens(ids0, table0, pe0, 3))))
    _untouched({"table": table, "pe": pe})


# ------------------------------------------------------------------------------------------------ wd_emb_combine
def _combine(time_ptr, label, y, ncls, T, B, ted, hi, lo, ld):
    N.check(N.lib().wd_emb_combine(time_ptr, None if label is None else label.data_ptr(), None if y is None else y.data_ptr(),
                                   ncls, T, B, ted, hi, lo, ld, _st()), "wd_emb_combine")


def _assert_planes_within(view, ref, what):
    ok, worst = E.within(_value(view), ref, E.PLANE_BOUND)
    print(f"{what}: err/bound {worst:.4f}")
    assert ok, (what, worst)


@pytest.mark.parametrize("form", ["label", "no_label", "clamped"])
@pytest.mark.parametrize("c", **E.params("wd_emb_combine"))
def test_emb_combine(c, form):
    T, B, ted, ncls = c["T"], c["B"], c["ted"], c["ncls"]
    time0, label0 = E.rand((T, ted), 190), E.rand((ncls, ted), 191)
    y0 = torch.randint(0, ncls, (B,), generator=torch.Generator().manual_seed(192))
    y0[0] = ncls - 1
    if form == "clamped":
        y0[0] = -5
        y0[-1] = 10 ** 6
    time_, label, y = _rows(time0), _rows(label0), _i64(y0)
    has = form != "no_label"
    ld = ted + 8
    buf, view = _planes_out(T * B, ted, ld)

    def launch(hi, lo):
        _combine(time_[1].data_ptr(), label[1] if has else None, y[1] if has else None, ncls if has else 0, T, B, ted, hi, lo, ld)

    launch(view[0].data_ptr(), view[1].data_ptr())
    torch.cuda.synchronize()
    G.assert_untouched(buf, view, "planes")
    G.assert_finite(view, "planes")
    _assert_planes_within(view, E.emb_combine(time0, label0 if has else None, y0, B), f"wd_emb_combine {form} {E.case_id(c)}")
    _untouched({"time": time_, "label": label})
    assert torch.equal(time_[1].cpu(), time0) and torch.equal(label[1].cpu(), label0)
    _i64_untouched(*y, "y")
    _hi_only(launch, T * B, ted, ld, view)


def test_emb_combine_in_two_chunks_at_a_row_offset():
    """As the engine tabulates: the second chunk reads ``time`` from its row 10 on and writes the planes from row 10 * B on."""
    T, B, ted, ncls = 19, 5, 256, 339
    time0, label0 = E.rand((T, ted), 195), E.rand((ncls, ted), 196)
    y0 = torch.randint(0, ncls, (B,), generator=torch.Generator().manual_seed(197))
    time_, label, y = _rows(time0), _rows(label0), _i64(y0)
    ld = ted + 8
    buf, view = _planes_out(T * B, ted, ld)
    for t0, nt in ((0, 10), (10, 9)):
        _combine(time_[1][t0].data_ptr(), label[1], y[1], ncls, nt, B, ted, view[0, t0 * B].data_ptr(), view[1, t0 * B].data_ptr(), ld)
    torch.cuda.synchronize()
    G.assert_untouched(buf, view, "planes")
    G.assert_finite(view, "planes")
    _assert_planes_within(view, E.emb_combine(time0, label0, y0, B), "wd_emb_combine in two chunks")
    one = _planes_out(T * B, ted, ld)
    _combine(time_[1].data_ptr(), label[1], y[1], ncls, T, B, ted, one[1][0].data_ptr(), one[1][1].data_ptr(), ld)
    torch.cuda.synchronize()
    assert torch.equal(_bits(view), _bits(one[1]))
    _untouched({"time": time_, "label": label})


# ------------------------------------------------------------------------------------------------ wd_timestep_embedding
@pytest.mark.parametrize("which", sorted(E.TEMB_T))
@pytest.mark.parametrize("dim", E.TEMB_DIMS)
def test_timestep_embedding(dim, which):
    t0 = torch.tensor(E.TEMB_T[which], dtype=torch.int64)
    batch, half, ld = t0.numel(), dim // 2, dim + 8
    freqs0 = E.temb_freqs(dim)
    t, freqs = _i64(t0), _flat(freqs0)
    buf, view = _planes_out(batch, dim, ld)

    def launch(hi, lo):
        N.check(N.lib().wd_timestep_embedding(t[1].data_ptr(), batch, freqs[1].data_ptr(), half, hi, lo, ld, _st()),
                "wd_timestep_embedding")

    launch(view[0].data_ptr(), view[1].data_ptr())
    torch.cuda.synchronize()
    G.assert_untouched(buf, view, "planes")
    G.assert_finite(view, "planes")
    err = float((_value(view) - E.timestep_embedding(t0, freqs0)).abs().max())
    print(f"wd_timestep_embedding dim {dim} {which}: max |err| {err:.3e}")
    assert err < E.TEMB_BOUND
    _same({"freqs": (freqs, freqs0)})
    _i64_untouched(*t, "t")
    _hi_only(launch, batch, dim, ld, view)


# ------------------------------------------------------------------------------------------------ wd_advance_timestep
@pytest.mark.parametrize("batch", E.ADVANCE_BATCH)
def test_advance_timestep(batch):
    for t, delta in E.ADVANCE_STEPS:
        td = _t_dev(t)
        buf, t64 = _i64(torch.full((batch,), -1, dtype=torch.int64))
        N.check(N.lib().wd_advance_timestep(td[1].data_ptr(), delta, t64.data_ptr(), batch, _st()), "wd_advance_timestep")
        torch.cuda.synchronize()
        want = E.advance(t, delta)
        G.assert_untouched(*td, "t_dev")
        _i64_untouched(buf, t64, "t64")
        assert int(td[1].item()) == want, (t, delta)
        assert torch.equal(t64.cpu(), torch.full((batch,), want, dtype=torch.int64)), (t, delta)


# ------------------------------------------------------------------------------------------------ wd_copy2d
def test_copy2d_between_two_pitched_windows_of_odd_width():
    rows, cols = 7, 19
    src0 = E.rand((rows, cols), 200).to(torch.bfloat16)
    src = G.pitched(src0, 40, 3, device=DEV)
    dst = G.guarded(rows, cols, 56, 5, torch.bfloat16, device=DEV)
    width = 2 * cols - 1  # the high byte of every row's last element is not copied
    N.check(N.lib().wd_copy2d(dst[1].data_ptr(), 2 * 56, src[1].data_ptr(), 2 * 40, width, rows, _st()), "wd_copy2d")
    torch.cuda.synchronize()
    G.assert_untouched(*dst, "dst")
    G.assert_untouched(*src, "src")
    assert torch.equal(_bits(src[1]), _bits(src0))
    got = dst[1].cpu().contiguous().view(torch.uint8).reshape(rows, 2 * cols)
    want = src0.contiguous().view(torch.uint8).reshape(rows, 2 * cols).clone()
    want[:, -1] = G.NAN16 >> 8
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ refusals
# One bad argument at a time: a pointer 4 bytes off the alignment its float4 / uint2 accesses need, or a pitch shorter than a row.
# Every call returns WD_EINVAL before anything is launched, and the poisoned outputs keep their pattern.
def _f32(n):
    return G.poisoned((1, n), torch.float32, DEV)


def _refusal_cases():
    B, n, ted, ncls, T = 2, 16, 8, 3, 2

    def ddpm(bad):
        x, eps, z, tab, td = _f32(B * n + 4), _f32(B * n + 4), _f32(B * n + 4), torch.ones(4, device=DEV), torch.ones(1, dtype=torch.int32, device=DEV)
        p = {k: v.data_ptr() + (4 if bad == k else 0) for k, v in dict(x=x, eps=eps, noise=z).items()}
        return (lambda: N.lib().wd_ddpm_step(p["x"], p["eps"], B, n, tab.data_ptr(), tab.data_ptr(), tab.data_ptr(), td.data_ptr(),
                                             p["noise"], 1, 0, _st())), [x]

    def cfg(bad):
        bufs = {k: _f32(B * n + 4) for k in ("x", "first", "second", "eps_out", "noise")}
        tab, td = torch.ones(4, device=DEV), torch.ones(1, dtype=torch.int32, device=DEV)
        p = {k: v.data_ptr() + (4 if bad == k else 0) for k, v in bufs.items()}
        return (lambda: N.lib().wd_ddpm_step_cfg(p["x"], p["first"], p["second"], 3.0, p["eps_out"], B, n, tab.data_ptr(),
                                                 tab.data_ptr(), tab.data_ptr(), td.data_ptr(), p["noise"], 1, 0, _st())), \
            [bufs["x"], bufs["eps_out"]]

    def randn(bad):
        out = _f32(B * n + 4)
        return (lambda: N.lib().wd_randn(out.data_ptr() + (4 if bad == "out" else 0), B, n, 1, 0, 0, _st())), [out]

    def select(bad):
        table, out, td = torch.ones(3 * B * n + 4, device=DEV), _f32(B * n + 4), torch.ones(1, dtype=torch.int32, device=DEV)
        return (lambda: N.lib().wd_select_rows(table.data_ptr() + (4 if bad == "table" else 0), td.data_ptr(), B, n, 3,
                                               out.data_ptr() + (4 if bad == "out" else 0), _st())), [out]

    def label_mix(bad):
        label, out = torch.ones(ncls * ted + 4, device=DEV), _f32(B * ted + 4)
        pairs, mix = torch.zeros(B, 2, dtype=torch.int32, device=DEV), torch.zeros(B, device=DEV)
        return (lambda: N.lib().wd_label_mix(label.data_ptr() + (4 if bad == "label" else 0), pairs.data_ptr(), mix.data_ptr(), ncls,
                                             B, ted, out.data_ptr() + (4 if bad == "out" else 0), _st())), [out]

    def combine(bad):
        time_, label = torch.ones(T * ted + 4, device=DEV), torch.ones(ncls * ted + 4, device=DEV)
        y = torch.zeros(B, dtype=torch.int64, device=DEV)
        pl = G.poisoned((2, T * B + 1, ted), torch.bfloat16, DEV)
        off = lambda k: 4 if bad == k else 0  # noqa: E731
        return (lambda: N.lib().wd_emb_combine(time_.data_ptr() + off("time"), label.data_ptr() + off("label"), y.data_ptr(), ncls, T,
                                               B, ted, pl[0].data_ptr() + off("out_hi"), pl[1].data_ptr() + off("out_lo"),
                                               ted - 4 if bad == "out_ld" else ted, _st())), [pl]

    def embed(bad):
        table, pe = torch.ones(5 * ted + 4, device=DEV), torch.ones(3 * ted + 4, device=DEV)
        ids = torch.zeros(6, dtype=torch.int64, device=DEV)
        pl = G.poisoned((2, 7, ted), torch.bfloat16, DEV)
        off = lambda k: 4 if bad == k else 0  # noqa: E731
        return (lambda: N.lib().wd_embed_tokens(ids.data_ptr(), 1, 6, 3, table.data_ptr() + off("table"), 5, ted,
                                                pe.data_ptr() + off("pe"), pl[0].data_ptr() + off("out_hi"),
                                                pl[1].data_ptr() + off("out_lo"), ted - 4 if bad == "out_ld" else ted, _st())), [pl]

    return {"wd_ddpm_step": (ddpm, ("x", "eps", "noise")),
            "wd_ddpm_step_cfg": (cfg, ("x", "first", "second", "eps_out", "noise")),
            "wd_randn": (randn, ("out",)),
            "wd_select_rows": (select, ("table", "out")),
            "wd_label_mix": (label_mix, ("label", "out")),
            "wd_emb_combine": (combine, ("time", "label", "out_hi", "out_lo", "out_ld")),
            "wd_embed_tokens": (embed, ("table", "pe", "out_hi", "out_lo", "out_ld"))}


_REFUSALS = [(fn, bad) for fn, (_, bads) in sorted(_refusal_cases().items()) for bad in bads]


@pytest.mark.parametrize("fn,bad", _REFUSALS, ids=[f"{fn}-{bad}" for fn, bad in _REFUSALS])
def test_entry_point_refuses_what_its_accesses_assume(fn, bad):
    make = _refusal_cases()[fn][0]
    call, outs = make(bad)
    assert call() == N.WD_EINVAL, (fn, bad)
    torch.cuda.synchronize()
    for o in outs:
        G.assert_untouched(o, (0, 0, 0, 0), f"{fn} output ({bad} refused)")
    good, outs = make(None)  # the same call with nothing wrong is accepted: it is that one argument that is refused
    assert good() == N.WD_OK, fn
    torch.cuda.synchronize()
