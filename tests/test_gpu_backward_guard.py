"""The non-GEMM backward building blocks (csrc/wd_bwd.hip) on PITCHED, GUARDED, RAGGED operands, as tests/test_gpu_pitch.py does for
the GEMM family: every operand a window of a buffer whose every other element is a NaN pattern (tests/_guard.py), every output and
scratch buffer a guarded window, checked after each launch for stores outside it (assert_untouched) and for values that came from
outside an operand's window or were never written (assert_finite).  Shapes: the smallest at which each branch of a kernel is live.

  * pure data movement (transposes, the planes of wd_dout_prep, wd_permute_dw, wd_pool2x2_sum, wd_add, single-occurrence rows of
    wd_embedding_bwd) is compared bit for bit; wd_split4 rounds to nearest even, so planes == _guard.split_planes(x);
  * column sums are compared element by element with fp64: |got - ref| <= 64 * 2^-24 * sum|x| of that column, times |scale| (the
    longest fp32 chain is 32 sequential adds per lane + 3 in colsum_stage1, 4 + 16 in dout_prep, stage 2 is fp64); with accumulate
    one more rounding of the stored value, 2^-24 * |result|.  Inputs have a non-zero column mean so that a dropped row shows;
  * GroupNorm / LayerNorm / attention backward against fp64 autograd at the tolerance of tests/test_gpu_backward.py (max_rel 3e-5),
    GEGLU at 2e-5 (wd_dout_prep_geglu 1e-5, as its test there); accumulate = 1 adds to RANDOM prior content."""
import ctypes as C
import functools
import struct

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests import _dropout_ref as R  # noqa: E402
from tests import _guard as G  # noqa: E402
from tests._common import max_rel  # noqa: E402
from worddiffusion_amd import _native as N  # noqa: E402
from worddiffusion_amd import dropout as DO  # noqa: E402
from worddiffusion_amd.engine import conv_gather_table  # noqa: E402

DEV = "cuda:0"
EPS24 = 2.0 ** -24
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NOTHING = (0, 0, 0, 0)  # the empty window: a buffer no launch may touch


def _st():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _sync():
    torch.cuda.synchronize()


def _run(name, *args):
    N.check(getattr(N.lib(), name)(*args, _st()), name)
    _sync()


def _refused(name, *args):
    assert getattr(N.lib(), name)(*args, _st()) == N.WD_EINVAL, name
    _sync()


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * int(k) for i, k in enumerate(key)) + 12345)


def _randn(g, *shape, mean=0.0, std=1.0):
    return torch.randn(*shape, generator=g) * std + mean


def _pit(x, extra, col0, g=2):
    """fp32 / int32 2-D operand as a window: (buffer, window, pitch)."""
    buf, view = G.pitched(x, x.shape[1] + extra, col0, g, DEV)
    return buf, view, buf.shape[-1]


def _vec(v, extra=8, col0=4):
    """A vector operand: one row, guard rows around it."""
    return G.pitched(v[None], v.numel() + extra, col0, 2, DEV)[1][0]


def _out(rows, cols, extra, col0, dtype=F32, planes=0, prior=None):
    """(buffer, window, pitch) of an output; prior: what the window holds before the launch (accumulate)."""
    buf, view = G.guarded(rows, cols, cols + extra, col0, dtype, 2, DEV, planes)
    if prior is not None:
        view.copy_(prior)
    return buf, view, buf.shape[-1]


def _flat(n, dtype=F32):
    return G.guarded_flat(n, dtype, 64, DEV)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _same_bits(got, want, name):
    assert got.shape == want.shape and got.dtype == want.dtype, name
    bad = _bits(got) != _bits(want)
    assert not bool(bad.any()), (f"{name}: {int(bad.sum())} element(s) differ, first at {tuple(int(i) for i in bad.nonzero()[0])}: "
                                 f"{got.cpu()[tuple(bad.nonzero()[0])].item()!r} != {want[tuple(bad.nonzero()[0])].item()!r}")


def _checked(outs):
    """outs: (name, buffer, window or None).  None: the buffer was not handed to the launch."""
    for name, buf, view in outs:
        G.assert_untouched(buf, NOTHING if view is None else view, name)
        if view is not None:
            G.assert_finite(view, name)


def _sums_close(got, ref, bound, name):
    """Element by element: |got - ref| <= bound (fp64 tensors of one shape)."""
    got, ref = got.detach().cpu().double(), ref.double()
    assert got.shape == ref.shape == bound.shape, name
    bad = ~((got - ref).abs() <= bound)
    err = ((got - ref).abs() / bound.clamp_min(1e-300))
    print(f"{name}: largest |got - ref| / bound = {float(err.max()):.3f}")
    assert not bool(bad.any()), (f"{name}: {int(bad.sum())} element(s) outside the bound, first at "
                                 f"{tuple(int(i) for i in bad.nonzero()[0])}: got {got[tuple(bad.nonzero()[0])].item()!r}, "
                                 f"want {ref[tuple(bad.nonzero()[0])].item()!r}")


def _tplanes(x, mpad):
    """[m][c] fp32 -> the transposed split planes [2][c][mpad], zero beyond m."""
    p = G.split_planes(x)
    t = torch.zeros(2, x.shape[1], mpad, dtype=BF16)
    t[:, :, :x.shape[0]] = p.transpose(1, 2)
    return t


# ------------------------------------------------------------------------------------------ wd_transpose_planes
@pytest.mark.parametrize("ld,col0,lo", [(76, 0, True), (75, 0, True), (76, 1, True), (76, 0, False)],
                         ids=["vector_body_scalar_last_quad", "odd_pitch_all_scalar", "misaligned_base", "no_lo_plane"])
def test_transpose_planes_fp32_input(ld, col0, lo):
    m, mpad, c = 130, 192, 70
    x = _randn(_gen(m, c), m, c)
    xb, xv = G.pitched(x, ld, col0, 2, DEV)
    ob, ov, _ = _out(c, mpad, 0, 0, BF16, planes=2)
    _run("wd_transpose_planes", xv.data_ptr(), None, 1, ld, c, None, 1, 0, 0, m, mpad, 0, ov[0].data_ptr(),
         ov[1].data_ptr() if lo else None)
    want = _tplanes(x, mpad)
    if lo:
        _checked([("transposed planes", ob, ov)])
        _same_bits(ov, want, "transposed planes")
    else:
        _checked([("transposed hi plane", ob[0], ov[0]), ("lo plane (not given)", ob[1], None)])
        _same_bits(ov[0], want[0], "transposed hi plane")
    assert not bool(_bits(ov[0])[:, m:].any())  # columns m .. mpad - 1: +0


def _gathered_reference(x, in_lo, tab, B, hw, c, mpad, tap_minor):
    p = G.split_planes(x)                                   # [2][B * hw][c]
    if not in_lo:
        p[1].zero_()
    t = torch.from_numpy(tab.astype(np.int64))              # [9][hw]
    src = (torch.arange(B)[None, :, None] * hw + t[:, None, :].clamp_min(0)).reshape(9, B * hw)
    ok = (t >= 0)[:, None, :].expand(9, B, hw).reshape(9, B * hw)
    gat = torch.where(ok[None, :, :, None], p[:, src], torch.zeros((), dtype=BF16))  # [2][9][m][c]
    gat = gat.permute(0, 3, 1, 2) if tap_minor else gat.permute(0, 1, 3, 2)           # [2][c][9][m] or [2][9][c][m]
    out = torch.zeros(2, 9 * c, mpad, dtype=BF16)
    out[:, :, :B * hw] = gat.reshape(2, 9 * c, B * hw)
    return out


@pytest.mark.parametrize("tap_minor", [0, 1])
@pytest.mark.parametrize("ld,col0,in_lo", [(76, 0, True), (76, 6, True), (76, 0, False)],
                         ids=["vector_body_scalar_last_quad", "pointer_off_the_8_byte_grid", "no_lo_input"])
def test_transpose_planes_plane_input_with_gather(ld, col0, in_lo, tap_minor):
    B, h, w, c, mpad = 2, 5, 7, 70, 128
    hw, m = h * w, B * h * w
    tab, ho, wo = conv_gather_table(h, w, "same")
    assert tab.shape == (9, hw) and (ho, wo) == (h, w) and int((tab < 0).sum()) > 0
    x = _randn(_gen(m, c, 9), m, c)
    xb, xv = G.pitched_planes(x, ld, col0, 2, DEV)
    tb, tv, _ = _pit(torch.from_numpy(tab.reshape(1, -1).copy()), 0, 0)
    ob, ov, _ = _out(9 * c, mpad, 0, 0, BF16, planes=2)
    _run("wd_transpose_planes", xv[0].data_ptr(), xv[1].data_ptr() if in_lo else None, 0, ld, c, tv.data_ptr(), 9, hw, hw, m, mpad,
         tap_minor, ov[0].data_ptr(), ov[1].data_ptr())
    _checked([("transposed tap planes", ob, ov)])
    _same_bits(ov, _gathered_reference(x, in_lo, tab, B, hw, c, mpad, tap_minor), "transposed tap planes")


def test_transpose_planes_contract():
    """mpad % 4 != 0 (the last 8-byte store of a row would run into the next channel's row) and taps without a table: refused,
    nothing launched."""
    m, c = 300, 8
    xb, xv, ld = _pit(_randn(_gen(m), m, c), 0, 0)
    ob, ov, _ = _out(9 * c, 304, 0, 0, BF16, planes=2)
    _refused("wd_transpose_planes", xv.data_ptr(), None, 1, ld, c, None, 1, 0, 0, m, 302, 0, ov[0].data_ptr(), ov[1].data_ptr())
    _refused("wd_transpose_planes", xv.data_ptr(), None, 1, ld, c, None, 9, 0, 0, m, 304, 0, ov[0].data_ptr(), ov[1].data_ptr())
    G.assert_untouched(ob, NOTHING, "output of a refused launch")


# ------------------------------------------------------------------------------------------ wd_dout_prep
_PREP_OUTS = {"pl": (1, 1, 0, 0, 0), "pl_hi": (1, 0, 0, 0, 0), "t": (0, 0, 1, 1, 0), "t_hi": (0, 0, 1, 0, 0), "colpart": (0, 0, 0, 0, 1),
              "all": (1, 1, 1, 1, 1)}


def _prep_buffers(m, n, npad, mpad, which):
    pb, pv, _ = _out(m, npad, 0, 0, BF16, planes=2)
    tb, tv, _ = _out(n, mpad, 0, 0, BF16, planes=2)
    cb, cv, _ = _out((mpad + 63) // 64, n, 0, 0)
    use = _PREP_OUTS[which]
    ptrs = [v.data_ptr() if u else None for v, u in zip((pv[0], pv[1], tv[0], tv[1], cv), use)]
    outs = [(f"{nm} plane {i}", b[i], v[i] if u else None) for nm, b, v, us in (("row-major", pb, pv, use[0:2]), ("transposed", tb, tv, use[2:4]))
            for i, u in enumerate(us)] + [("column sums", cb, cv if use[4] else None)]
    return (pv, tv, cv), ptrs, outs, use


@pytest.mark.parametrize("npad", [72, 136])
@pytest.mark.parametrize("which", sorted(_PREP_OUTS))
def test_dout_prep_ragged_columns_and_single_outputs(which, npad):
    """n = 70: the last column quad of a row holds two values (the scalar tail); npad = 136: the column tile 128..135 lies wholly in
    the zero padding of the row-major planes; the last 64-row block sums two rows."""
    m, mpad, n = 130, 192, 70
    x = _randn(_gen(m, n, 3), m, n, mean=0.75)
    xb, xv, ld = _pit(x, 6, 4)
    (pv, tv, cv), ptrs, outs, use = _prep_buffers(m, n, npad, mpad, which)
    _run("wd_dout_prep", xv.data_ptr(), ld, m, n, npad, mpad, *ptrs)
    _checked(outs)
    pl = torch.zeros(2, m, npad, dtype=BF16)
    pl[:, :, :n] = G.split_planes(x)
    tp = _tplanes(x, mpad)
    for i in range(2):
        if use[i]:
            _same_bits(pv[i], pl[i], f"row-major plane {i}")
        if use[2 + i]:
            _same_bits(tv[i], tp[i], f"transposed plane {i}")
    if use[4]:
        xp = torch.zeros(mpad, n, dtype=F64)
        xp[:m] = x.double()
        blocks = xp.reshape(mpad // 64, 64, n)
        _sums_close(cv, blocks.sum(1), 64 * EPS24 * blocks.abs().sum(1), "64-row column sums")


def test_dout_prep_contract():
    m, mpad, n = 130, 192, 70
    x = _randn(_gen(m, n), m, n)
    xb, xv, ld = _pit(x, 6, 4)
    ub, uv, uld = _pit(x, 6, 1)  # a base pointer off the 16-byte grid
    (pv, tv, cv), ptrs, outs, _ = _prep_buffers(m, n, 72, mpad, "all")
    _refused("wd_dout_prep", xv.data_ptr(), ld, m, n, 70, mpad, *ptrs)
    _refused("wd_dout_prep", uv.data_ptr(), uld, m, n, 72, mpad, *ptrs)
    for name, buf, _ in outs:
        G.assert_untouched(buf, NOTHING, name)


@functools.lru_cache(maxsize=None)
def _geglu_case(m, inner):
    g = _gen(m, inner, 7)
    u, dh = _randn(g, m, 2 * inner), _randn(g, m, inner, mean=0.5)
    ur = u.double().requires_grad_(True)
    hh = ur[:, :inner] * F.gelu(ur[:, inner:])
    hh.backward(dh.double())
    return u, dh, hh.detach(), ur.grad


@pytest.mark.parametrize("which", sorted(_PREP_OUTS))
def test_dout_prep_geglu_pitched_and_single_outputs(which):
    m, inner, mpad = 130, 64, 192
    n = 2 * inner
    u, dh, _, du = _geglu_case(m, inner)
    ub, uv, u_ld = _pit(u, 8, 4)
    hb, hv, dh_ld = _pit(dh, 8, 4)
    assert (u_ld, dh_ld) == (136, 72)
    (pv, tv, cv), ptrs, outs, use = _prep_buffers(m, n, n, mpad, which)
    _run("wd_dout_prep_geglu", uv.data_ptr(), u_ld, hv.data_ptr(), dh_ld, m, inner, mpad, *ptrs)
    _checked(outs)
    if use[0] and use[1]:
        assert max_rel(pv[0].float().cpu() + pv[1].float().cpu(), du) < 1e-5
    elif use[0]:
        assert max_rel(pv[0].float().cpu(), du) < 2.0 ** -8  # the hi plane alone: bf16 of the value
    if use[2]:
        t = tv[0].float().cpu() + (tv[1].float().cpu() if use[3] else 0)
        assert max_rel(t[:, :m].t(), du) < (1e-5 if use[3] else 2.0 ** -8)
        for i in range(1 + use[3]):
            assert not bool(_bits(tv[i])[:, m:].any())
    if which == "all":
        _same_bits(tv[:, :, :m].transpose(1, 2).contiguous(), pv.cpu(), "transposed planes against the row-major planes")
    if use[4]:
        dp = torch.zeros(mpad, n, dtype=F64)
        dp[:m] = du
        assert max_rel(cv.cpu(), dp.reshape(mpad // 64, 64, n).sum(1)) < 1e-5


# ------------------------------------------------------------------------------------------ column sums
def _colsum_bound(ref_abs, scale, result=None):
    b = 64 * EPS24 * ref_abs * abs(scale)
    return b if result is None else b + EPS24 * result.abs()


@pytest.mark.parametrize("extra,col0", [(2, 0), (1, 0), (6, 1)], ids=["vector", "odd_pitch_scalar", "misaligned_base_scalar"])
def test_colsum_segments_blocks_and_ragged_width(extra, col0):
    """Three segments (the last of 20 rows), two 128-row blocks per segment (the second of 12 or 0 rows), two 256-column blocks and
    a last column quad of two; scratch exactly as large as the entry point demands."""
    rows, seg, c, out_ld, scale = 300, 140, 262, 270, 0.5
    nseg, nblk = 3, 2
    x = _randn(_gen(rows, c, extra), rows, c, mean=0.5)
    xb, xv, ld = _pit(x, extra, col0)
    xd = torch.zeros(nseg * seg, c, dtype=F64)
    xd[:rows] = x.double()
    ref, ref_abs = xd.reshape(nseg, seg, c).sum(1), xd.reshape(nseg, seg, c).abs().sum(1)
    sb, sv = _flat(nseg * nblk * c)
    prior = _randn(_gen(c), nseg, c)
    for acc in (0, 1):
        ob, ov, old = _out(nseg, c, out_ld - c, 4, prior=prior if acc else None)
        assert old == out_ld
        _run("wd_colsum", xv.data_ptr(), ld, rows, c, seg, ov.data_ptr(), out_ld, acc, scale, sv.data_ptr(), sv.numel())
        _checked([("column sums", ob, ov), ("scratch", sb, sv)])
        want = ref * scale + (prior.double() if acc else 0)
        _sums_close(ov, want, _colsum_bound(ref_abs, scale, want if acc else None), f"column sums (accumulate {acc})")
    ob, ov, _ = _out(nseg, c, out_ld - c, 4)  # scratch one float short: refused, nothing launched
    sb, sv = _flat(nseg * nblk * c)
    _refused("wd_colsum", xv.data_ptr(), ld, rows, c, seg, ov.data_ptr(), out_ld, 0, scale, sv.data_ptr(), sv.numel() - 1)
    G.assert_untouched(ob, NOTHING, "column sums of a refused launch")
    G.assert_untouched(sb, NOTHING, "scratch of a refused launch")


@pytest.mark.parametrize("nblk", [1, 16, 17])
def test_colsum_finish_film_gradient_form(nblk):
    nseg, c, out_ld = 3, 70, 80
    part = _randn(_gen(nblk, c), nseg * nblk, c, mean=0.5)
    pb, pv, _ = _pit(part, 0, 0)
    ref, ref_abs = part.double().reshape(nseg, nblk, c).sum(1), part.double().reshape(nseg, nblk, c).abs().sum(1)
    prior = _randn(_gen(c, nblk), nseg, c)
    for acc, scale in ((0, 1.0), (1, -0.25)):
        ob, ov, _ = _out(nseg, c, out_ld - c, 4, prior=prior if acc else None)
        _run("wd_colsum_finish", pv.data_ptr(), nblk, c, nseg, ov.data_ptr(), out_ld, acc, scale)
        _checked([("finished sums", ob, ov)])
        want = ref * scale + (prior.double() if acc else 0)
        _sums_close(ov, want, _colsum_bound(ref_abs, scale, want if acc else None), f"finished sums (accumulate {acc})")


def test_colsum_finish_multi_one_launch_of_mixed_entries():
    """Entries of 1 .. 130 partial rows (the four-in-flight loop runs 0, 1 and 2 rounds, for one lane or for all, with and without
    a remainder) and of widths below the widest (whole column tiles return early); the outputs tile one guarded buffer."""
    lib = N.lib()
    nblks, widths = (1, 16, 17, 49, 64, 65, 130), (70, 1, 16, 17, 70, 16, 17)
    scales, accs = (1.0, 0.5, -2.0, 1.0, 0.25, 1.0, -1.0), (0, 1, 0, 1, 1, 0, 1)
    assert lib.wd_colsum_entry_bytes() == 40
    g = _gen(130, 70)
    ob, ov = _flat(sum(widths))
    prior = _randn(g, sum(widths))
    ov.copy_(prior)
    keep, recs, wants, bounds, off = [], [], [], [], 0
    for nblk, c, scale, acc in zip(nblks, widths, scales, accs):
        part = _randn(g, nblk, c, mean=0.5)
        pb, pv, ld = _pit(part, 5, 2)
        keep.append(pb)
        recs.append(struct.pack("<QQiiiifi", pv.data_ptr(), ov[off:off + c].data_ptr(), nblk, c, ld, acc, scale, 0))
        want = part.double().sum(0) * scale + (prior[off:off + c].double() if acc else 0)
        wants.append(want)
        bounds.append(_colsum_bound(part.double().abs().sum(0), scale, want if acc else None))
        off += c
    table = torch.frombuffer(bytearray(b"".join(recs)), dtype=torch.uint8).to(DEV)
    _run("wd_colsum_finish_multi", table.data_ptr(), len(recs), max(widths))
    _checked([("parameter gradients", ob, ov)])
    _sums_close(ov, torch.cat(wants), torch.cat(bounds), "parameter gradients")


# ------------------------------------------------------------------------------------------ GroupNorm backward
@functools.lru_cache(maxsize=None)
def _gn_case(B, hw, cs, silu, eps=1e-5):
    """fp64 autograd of GroupNorm32(+SiLU) over the channel concat of the sources: inputs, dz, gamma, beta and every gradient."""
    g = _gen(B, hw, sum(cs), silu)
    ctot = sum(cs)
    xs = [_randn(g, B * hw, c, mean=0.5, std=2.0) for c in cs]
    gamma, beta = _randn(g, ctot).double().requires_grad_(True), _randn(g, ctot).double().requires_grad_(True)
    xr = [x.double().requires_grad_(True) for x in xs]
    y = F.group_norm(torch.cat(xr, 1).reshape(B, hw, ctot).permute(0, 2, 1), 32, gamma, beta, eps)
    if silu:
        y = F.silu(y)
    dz = _randn(g, B * hw, ctot)
    y.permute(0, 2, 1).reshape(B * hw, ctot).backward(dz.double())
    return xs, dz, gamma.detach().float(), beta.detach().float(), [x.grad for x in xr], gamma.grad, beta.grad


class _GnLaunch:
    """One source of a GroupNorm backward on pitched, guarded operands: x at pitch c + 8, dz inside a [B * hw][ctot + 8] matrix,
    gamma / beta inside longer vectors, dx at pitch c + 4, sums exactly [B][chunks][2][c]."""

    def __init__(self, B, hw, cs, src, x, dz, gamma, beta, eps=1e-5):
        lib = N.lib()
        self.B, self.hw, self.c, self.eps = B, hw, cs[src], eps
        c, ctot = cs[src], sum(cs)
        self.off, self.cpg, self.pcpg = sum(cs[:src]), ctot // 32, cs[src] // 32
        self.nck, self.nb = lib.wd_gn_nchunk(hw), lib.wd_gn_bwd_nchunk(hw)
        self.xb, self.xv, self.ld = _pit(x, 8, 4)
        self.zb, self.zv, self.dz_ld = _pit(dz, 8, 4)
        self.gam, self.bet = _vec(gamma), _vec(beta)
        self.pb, self.part = G.guarded(B * self.nck, 2 * (c // self.pcpg), 2 * (c // self.pcpg), 0, F64, 2, DEV)
        _run("wd_gn_stats", self.xv.data_ptr(), self.ld, B, hw, c, self.pcpg, self.part.data_ptr())
        _checked([("forward statistics", self.pb, self.part)])

    def common(self, silu, dz=None, **kw):
        a = dict(hw=self.hw, c=self.c, cpg=self.cpg, pcpg=self.pcpg)
        a.update(kw)
        return ((self.xv.data_ptr(), self.ld, (self.zv if dz is None else dz).data_ptr(), self.dz_ld, self.off, self.B, a["hw"], a["c"],
                 a["cpg"], self.part.data_ptr(), self.nck, a["pcpg"], self.gam.data_ptr(), self.bet.data_ptr(), self.off, self.eps, silu))

    def dx(self, prior):
        return _out(self.B * self.hw, self.c, 4, 4, prior=prior)

    def two_pass(self, silu, prior, dz=None, tail=(), suffix=""):
        sb, sv = _flat(self.B * self.nb * 2 * self.c)
        ob, ov, dx_ld = self.dx(prior)
        _run("wd_gn_bwd_stats" + suffix, *self.common(silu, dz), sv.data_ptr(), *tail)
        _checked([("sums", sb, sv)])
        _run("wd_gn_bwd_apply" + suffix, *self.common(silu, dz), sv.data_ptr(), ov.data_ptr(), dx_ld, int(prior is not None), *tail)
        _checked([("sums", sb, sv), ("dx", ob, ov)])
        return sv.view(self.B, self.nb, 2, self.c).cpu(), ov.cpu()

    def one_pass(self, silu, prior, dz=None, tail=(), suffix=""):
        assert N.lib().wd_gn_bwd_fused_supported(self.hw, self.c, self.cpg)
        sb, sv = _flat(self.B * 2 * self.c)
        ob, ov, dx_ld = self.dx(prior)
        _run("wd_gn_bwd_fused" + suffix, *self.common(silu, dz), sv.data_ptr(), ov.data_ptr(), dx_ld, int(prior is not None), *tail)
        _checked([("sums", sb, sv), ("dx", ob, ov)])
        return sv.view(self.B, 1, 2, self.c).cpu(), ov.cpu()


def _gn_check(L, src, silu, acc, case):
    xs, dz, gamma, beta, dxs, dgamma, dbeta = case
    c, off = L.c, L.off
    prior = _randn(_gen(src, silu, c), L.B * L.hw, c) if acc else None
    base = prior if acc else 0
    sums, dx = L.two_pass(silu, prior)
    assert max_rel(dx - base, dxs[src]) < 3e-5
    tot = sums.double().sum((0, 1))  # [d beta | d gamma]
    assert max_rel(tot[0], dbeta[off:off + c]) < 3e-5 and max_rel(tot[1], dgamma[off:off + c]) < 3e-5
    sums1, dx1 = L.one_pass(silu, prior)
    assert max_rel(dx1 - base, dxs[src]) < 3e-5
    assert max_rel(sums1.sum((0, 1)), sums.sum((0, 1))) < 1e-5
    tot1 = sums1.double().sum((0, 1))
    assert max_rel(tot1[0], dbeta[off:off + c]) < 3e-5 and max_rel(tot1[1], dgamma[off:off + c]) < 3e-5


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("silu", [0, 1])
@pytest.mark.parametrize("src", [0, 1])
def test_groupnorm_backward_both_sources_pitched(src, silu, acc):
    """A decoder ResBlock's norm over (320 | 320) channels at hw = 35 (no multiple of the 32 / 16 / 25 token chunks of the three
    kernels): source 1 reads dz, gamma and beta at offset 320, and both read statistics kept per 10 channels under groups of 20."""
    B, hw, cs = 2, 35, (320, 320)
    case = _gn_case(B, hw, cs, silu)
    L = _GnLaunch(B, hw, cs, src, case[0][src], case[1], case[2], case[3])
    assert (L.ld, L.cpg, L.pcpg, L.off) == (328, 20, 10, 320 * src)
    _gn_check(L, src, silu, acc, case)


@pytest.mark.parametrize("acc", [0, 1])
def test_groupnorm_backward_generic_apply_branch(acc):
    """c = 1280: more channel quads than the 256 threads of gn_bwd_apply_kernel - its loop over (token, quad) pairs."""
    B, hw, cs = 2, 20, (1280,)
    case = _gn_case(B, hw, cs, 1)
    L = _GnLaunch(B, hw, cs, 0, case[0][0], case[1], case[2], case[3])
    assert (L.cpg, L.pcpg) == (40, 40) and L.c // 4 > 256
    _gn_check(L, 0, 1, acc, case)


def test_groupnorm_backward_contract():
    """Zero cpg, part_cpg or hw: WD_EINVAL from all three entry points (not a division by zero on the host), nothing launched."""
    B, hw, cs = 2, 35, (320, 320)
    case = _gn_case(B, hw, cs, 1)
    L = _GnLaunch(B, hw, cs, 1, case[0][1], case[1], case[2], case[3])
    sb, sv = _flat(B * L.nb * 2 * L.c)
    ob, ov, dx_ld = L.dx(None)
    for kw in (dict(cpg=0), dict(pcpg=0), dict(hw=0)):
        _refused("wd_gn_bwd_stats", *L.common(1, **kw), sv.data_ptr())
        _refused("wd_gn_bwd_apply", *L.common(1, **kw), sv.data_ptr(), ov.data_ptr(), dx_ld, 0)
        _refused("wd_gn_bwd_fused", *L.common(1, **kw), sv.data_ptr(), ov.data_ptr(), dx_ld, 0)
    G.assert_untouched(sb, NOTHING, "sums")
    G.assert_untouched(ob, NOTHING, "dx")


SEED, LAYER, ROW_BASE, ROW_BASE_DEV = 1234, 5, 5, 2


@pytest.mark.parametrize("acc", [0, 1])
def test_groupnorm_backward_dropout_second_source_pitched(acc):
    """wd_gn_bwd_*_dropout at p = 0.5 on the second source (offsets 320, pitched x / dz / dx): bit for bit the plain kernels on a dz
    masked beforehand - the mask is indexed by the channel inside the norm, not by the offsets."""
    B, hw, cs, src, silu, p = 2, 35, (320, 320), 1, 1, 0.5
    case = _gn_case(B, hw, cs, silu)
    xs, dz = case[0], case[1]
    L = _GnLaunch(B, hw, cs, src, xs[src], dz, case[2], case[3])
    c, off = L.c, L.off
    keep = R.keep_mask(SEED, ROW_BASE + ROW_BASE_DEV, B, hw, c, LAYER, p).reshape(B * hw, c)
    pre = dz.clone()
    pre[:, off:off + c] = torch.from_numpy(np.where(keep, dz[:, off:off + c].numpy() * R.scale(p), np.float32(0.0)))
    assert pre.dtype == F32 and 0.4 < float(keep.mean()) < 0.6
    qb, qv, q_ld = _pit(pre, 8, 4)
    assert q_ld == L.dz_ld
    row_dev = torch.tensor([ROW_BASE_DEV], dtype=torch.int64, device=DEV)
    d = DO.WdDropout()
    d.seed, d.row_base, d.row_base_dev = SEED, ROW_BASE, row_dev.data_ptr()
    d.tag, d.thr, d.scale = R.tag(LAYER), R.threshold(p), float(R.scale(p))
    prior = _randn(_gen(c, acc), B * hw, c) if acc else None
    s0, dx0 = L.two_pass(silu, prior, dz=qv)
    s1, dx1 = L.two_pass(silu, prior, tail=(C.byref(d),), suffix="_dropout")
    _same_bits(s1, s0, "two-pass sums")
    _same_bits(dx1, dx0, "two-pass dx")
    s0, dx0 = L.one_pass(silu, prior, dz=qv)
    s1, dx1 = L.one_pass(silu, prior, tail=(C.byref(d),), suffix="_dropout")
    _same_bits(s1, s0, "fused sums")
    _same_bits(dx1, dx0, "fused dx")
    assert max_rel(dx0 - (prior if acc else 0), case[4][src]) > 1e-2  # (the mask changed the gradient: it was applied)


# ------------------------------------------------------------------------------------------ LayerNorm backward
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("rows,c", [(17, 516), (3, 2048), (1, 4), (33, 320)])
def test_layernorm_backward_pitched(rows, c, acc):
    """c = 516 and 2048: the eight-float4 instantiation (512 < c <= 2048), its first width and its last; c = 4: one lane; 17 and 33
    rows: a second and third block with one row."""
    lib = N.lib()
    g = _gen(rows, c)
    x, dy, ga = _randn(g, rows, c, mean=1.0, std=3.0), _randn(g, rows, c), _randn(g, c)
    xr, gr = x.double().requires_grad_(True), ga.double().requires_grad_(True)
    br = torch.zeros(c, dtype=F64, requires_grad=True)
    F.layer_norm(xr, (c,), gr, br, 1e-5).backward(dy.double())
    nblk = lib.wd_layernorm_bwd_nblk(rows)
    assert nblk == (rows + 15) // 16
    xb, xv, ld = _pit(x, 4, 4)
    yb, yv, dy_ld = _pit(dy, 8, 4)
    prior = _randn(g, rows, c) if acc else None
    ob, ov, dx_ld = _out(rows, c, 12, 4, prior=prior)
    cb, cv = _flat(nblk * 2 * c)
    gv = _vec(ga)
    _run("wd_layernorm_bwd", xv.data_ptr(), ld, yv.data_ptr(), dy_ld, rows, c, gv.data_ptr(), 1e-5, ov.data_ptr(), dx_ld, acc,
         cv.data_ptr())
    _checked([("dx", ob, ov), ("column partials", cb, cv)])
    assert max_rel(ov.cpu() - (prior if acc else 0), xr.grad) < 3e-5
    tot = cv.view(nblk, 2, c).cpu().double().sum(0)  # [d gamma | d beta]
    assert max_rel(tot[0], gr.grad) < 3e-5 and max_rel(tot[1], br.grad) < 3e-5


@pytest.mark.parametrize("c", [2052, 6])
def test_layernorm_backward_contract(c):
    rows = 3
    wide = (c + 3) // 4 * 4 + 4  # a legal pitch: only c is at fault
    xb, xv, ld = _pit(torch.ones(rows, wide), 0, 0)
    ob, ov, dx_ld = _out(rows, wide, 0, 0)
    cb, cv = _flat(2 * c)
    _refused("wd_layernorm_bwd", xv.data_ptr(), ld, xv.data_ptr(), ld, rows, c, xv.data_ptr(), 1e-5, ov.data_ptr(), dx_ld, 0, cv.data_ptr())
    G.assert_untouched(ob, NOTHING, "dx")
    G.assert_untouched(cb, NOTHING, "column partials")


# ------------------------------------------------------------------------------------------ attention backward
def _attn_case(B, H, nq, nk, d, scale):
    g = _gen(B, H, nq, nk, d)
    inner = H * d
    q, k, v = (_randn(g, B * n, inner, std=0.5) for n in (nq, nk, nk))
    do = _randn(g, B * nq, inner)
    qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))

    def heads(t, n):
        return t.reshape(B, n, H, d).permute(0, 2, 1, 3)

    att = torch.softmax(heads(qr, nq) @ heads(kr, nk).transpose(-1, -2) * scale, -1)
    (att @ heads(vr, nk)).permute(0, 2, 1, 3).reshape(B * nq, inner).backward(do.double())
    return q, k, v, do, qr.grad, kr.grad, vr.grad


@pytest.mark.parametrize("B,H,nq,nk,d", [(2, 3, 70, 7, 20), (2, 4, 5, 16, 12), (1, 8, 20, 10, 80), (2, 4, 33, 1, 16)],
                         ids=["fallback_3_heads_d20", "fallback_16_keys", "q4_thread_cap_512", "q4_one_key"])
def test_attention_backward_small_fallback_and_edges(B, H, nq, nk, d):
    """d % 16 != 0 or 256 % (4 heads) != 0: attn_bwd_small_kernel (one thread per (token, head)); inner = 640: the q4 kernel with
    its block capped at 512 threads; nk = 16 and 1: the two ends of the key range."""
    lib = N.lib()
    scale = d ** -0.5
    inner = H * d
    q, k, v, do, dq_ref, dk_ref, dv_ref = _attn_case(B, H, nq, nk, d, scale)
    nwg = lib.wd_attention_bwd_small_nwg(H, nq, nk, d)
    assert nwg > 0
    (qb, qv, ldq), (kb, kv, ldk), (vb, vv, ldv), (gb, gv, ldo) = _pit(q, 4, 4), _pit(k, 8, 4), _pit(v, 12, 8), _pit(do, 4, 0)
    ob, ov, lddq = _out(B * nq, inner, 8, 4)
    pb, pv = _flat(B * nwg * nk * 2 * inner)
    nw = C.c_int(0)
    N.check(lib.wd_attention_bwd_small(qv.data_ptr(), ldq, kv.data_ptr(), ldk, vv.data_ptr(), ldv, gv.data_ptr(), ldo, B, H, nq, nk, d,
                                       scale, ov.data_ptr(), lddq, pv.data_ptr(), C.byref(nw), _st()), "wd_attention_bwd_small")
    _sync()
    assert nw.value == nwg
    _checked([("dq", ob, ov), ("dK / dV partials", pb, pv)])
    assert max_rel(ov.cpu(), dq_ref) < 3e-5
    dkv = pv.view(B, nwg, nk, 2, inner).cpu().double().sum(1)
    assert max_rel(dkv[:, :, 0].reshape(B * nk, inner), dk_ref) < 3e-5
    assert max_rel(dkv[:, :, 1].reshape(B * nk, inner), dv_ref) < 3e-5


def test_attention_backward_small_contract():
    B, H, nq, nk, d = 1, 4, 8, 17, 16
    inner = H * d
    xb, xv, ld = _pit(torch.ones(B * nk, inner), 0, 0)
    ob, ov, lddq = _out(B * nq, inner, 0, 0)
    pb, pv = _flat(B * nk * 2 * inner)
    assert N.lib().wd_attention_bwd_small(xv.data_ptr(), ld, xv.data_ptr(), ld, xv.data_ptr(), ld, xv.data_ptr(), ld, B, H, nq, nk, d, 0.25,
                                          ov.data_ptr(), lddq, pv.data_ptr(), None, _st()) == N.WD_EINVAL
    _sync()
    G.assert_untouched(ob, NOTHING, "dq")
    G.assert_untouched(pb, NOTHING, "dK / dV partials")


@pytest.mark.parametrize("nk", [64, 65])
def test_attention_backward_generic_pitched(nk):
    """nk = 64: every lane holds one key; 65: lane 0 holds a second.  Scratch of exactly wd_attention_bwd_scratch_floats."""
    lib = N.lib()
    B, H, nq, d = 2, 2, 9, 20
    scale, inner = d ** -0.5, H * d
    q, k, v, do, dq_ref, dk_ref, dv_ref = _attn_case(B, H, nq, nk, d, scale)
    (qb, qv, ldq), (kb, kv, ldk), (vb, vv, ldv), (gb, gv, ldo) = _pit(q, 3, 1), _pit(k, 8, 4), _pit(v, 12, 8), _pit(do, 5, 2)
    (ab, av, lddq), (bb, bv, lddk), (cb, cv, lddv) = _out(B * nq, inner, 7, 3), _out(B * nk, inner, 5, 2), _out(B * nk, inner, 9, 6)
    nscr = lib.wd_attention_bwd_scratch_floats(B, H, nq, nk)
    assert nscr == 2 * B * H * nq * nk
    sb, sv = _flat(nscr)
    args = (qv.data_ptr(), ldq, kv.data_ptr(), ldk, vv.data_ptr(), ldv, gv.data_ptr(), ldo, B, H, nq, nk, d, scale, av.data_ptr(), lddq,
            bv.data_ptr(), lddk, cv.data_ptr(), lddv, sv.data_ptr())
    _refused("wd_attention_bwd", *args, nscr - 1)
    for name, buf in (("dq", ab), ("dk", bb), ("dv", cb), ("scratch", sb)):
        G.assert_untouched(buf, NOTHING, name)
    _run("wd_attention_bwd", *args, nscr)
    _checked([("dq", ab, av), ("dk", bb, bv), ("dv", cb, cv), ("scratch", sb, sv)])
    assert max_rel(av.cpu(), dq_ref) < 3e-5 and max_rel(bv.cpu(), dk_ref) < 3e-5 and max_rel(cv.cpu(), dv_ref) < 3e-5


# ------------------------------------------------------------------------------------------ the small kernels
def test_pool2x2_sum_odd_map():
    B, h, w, c = 2, 3, 5, 12
    x = _randn(_gen(h, w, c), B, 2 * h, 2 * w, c)
    xb, xv, _ = _pit(x.reshape(-1, c), 0, 0)
    ob, ov, _ = _out(B * h * w, c, 0, 0)
    _run("wd_pool2x2_sum", xv.data_ptr(), B, h, w, c, ov.data_ptr())
    _checked([("pooled map", ob, ov)])
    want = (x[:, 0::2, 0::2] + x[:, 0::2, 1::2]) + (x[:, 1::2, 0::2] + x[:, 1::2, 1::2])  # the kernel's order, in fp32
    _same_bits(ov.cpu(), want.reshape(-1, c), "pooled map")


def test_embedding_backward_int32_ids_pitched_rows_assign():
    """int32 ids, d at pitch 44 for 40 columns, accumulate = 0 onto poison: a row nobody names is +0, a row named once is the bits
    of its d row, a row named k times is within (k - 1) roundings of the fp64 sum."""
    vocab, c = 11, 40
    ids = torch.tensor([3, 0, 3, 7, 3, 0, 10], dtype=torch.int32)
    d = _randn(_gen(vocab, c), ids.numel(), c, mean=0.5)
    ib, iv, _ = _pit(ids[None], 0, 0)
    db, dv, ld = _pit(d, 4, 0)
    assert ld == 44
    ob, ov, _ = _out(vocab, c, 0, 0)
    _run("wd_embedding_bwd", iv.data_ptr(), 0, ids.numel(), dv.data_ptr(), ld, vocab, c, ov.data_ptr(), 0)
    _checked([("table gradient", ob, ov)])
    onehot = (ids[:, None] == torch.arange(vocab)[None]).double()  # [rows][vocab]
    ref, ref_abs, count = onehot.t() @ d.double(), onehot.t() @ d.double().abs(), onehot.sum(0)
    _sums_close(ov, ref, (count - 1).clamp_min(0)[:, None] * EPS24 * ref_abs, "table gradient")
    _same_bits(ov[[7, 10, 1]].cpu(), torch.stack([d[3], d[6], torch.zeros(c)]), "rows named once / never")


@pytest.mark.parametrize("n", [3, 1027])
def test_add_ragged_length(n):
    g = _gen(n)
    a, b = _randn(g, n), _randn(g, n)
    ab, av = _flat(n)
    av.copy_(a)
    bb, bv = _flat(n)
    bv.copy_(b)
    _run("wd_add", av.data_ptr(), bv.data_ptr(), n)
    _checked([("dst", ab, av)])
    _same_bits(av.cpu(), a + b, "dst")


@pytest.mark.parametrize("ntaps", [1, 9])
def test_permute_dw_pitched_rows(ntaps):
    n, c = 5, 6
    packed = _randn(_gen(n, c, ntaps), n, ntaps * c)
    pb, pv, ld = _pit(packed, 3, 2)
    ob, ov, _ = _out(n, c * ntaps, 0, 0)
    _run("wd_permute_dw", pv.data_ptr(), ld, n, c, ntaps, ov.data_ptr())
    _checked([("OIHW gradient", ob, ov)])
    _same_bits(ov.cpu(), packed.reshape(n, ntaps, c).permute(0, 2, 1).reshape(n, c * ntaps).contiguous(), "OIHW gradient")


def test_geglu_forward_backward_and_silu_backward_guarded():
    rows, inner = 37, 20
    u, dh, hh, du_ref = _geglu_case(rows, inner)
    ub, uv, u_ld = _pit(u, 4, 4)
    hb, hv, dh_ld = _pit(dh, 8, 4)
    p2b, p2v, out_ld = _out(rows, inner, 8, 4, BF16, planes=2)
    _run("wd_geglu_fwd", uv.data_ptr(), u_ld, rows, inner, p2v[0].data_ptr(), p2v[1].data_ptr(), out_ld)
    _checked([("GEGLU planes", p2b, p2v)])
    assert max_rel(p2v[0].float().cpu() + p2v[1].float().cpu(), hh) < 2e-5
    p1b, p1v, _ = _out(rows, inner, 8, 4, BF16, planes=2)
    _run("wd_geglu_fwd", uv.data_ptr(), u_ld, rows, inner, p1v[0].data_ptr(), None, out_ld)
    _checked([("GEGLU hi plane", p1b[0], p1v[0]), ("lo plane (not given)", p1b[1], None)])
    _same_bits(p1v[0], p2v[0], "hi plane without a lo plane")
    ob, ov, du_ld = _out(rows, 2 * inner, 5, 3)
    _run("wd_geglu_bwd", uv.data_ptr(), u_ld, hv.data_ptr(), dh_ld, rows, inner, ov.data_ptr(), du_ld)
    _checked([("d u", ob, ov)])
    assert max_rel(ov.cpu(), du_ref) < 2e-5
    n = 5001
    g = _gen(n)
    pre, dact = _randn(g, n), _randn(g, n)
    pr = pre.double().requires_grad_(True)
    F.silu(pr).backward(dact.double())
    (ab, av), (bb, bv), (cb, cv) = _flat(n), _flat(n), _flat(n)
    av.copy_(pre)
    bv.copy_(dact)
    _run("wd_silu_bwd", av.data_ptr(), bv.data_ptr(), n, cv.data_ptr())
    _checked([("d pre", cb, cv)])
    assert max_rel(cv.cpu(), pr.grad) < 2e-5
