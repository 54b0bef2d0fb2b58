"""The weight-gradient kernel (csrc/wd_dw.hip: wd_dw, wd_dw_group) on GUARDED, SLICED and GROUPED inputs, as tests/test_gpu_pitch.py
does for the GEMM family: the planes of d(output) and of the layer input are windows of buffers whose every other element is a NaN
pattern (tests/_guard.py: guard rows 2, d at column 8 of pitch n + 24, x at column 16 of pitch c + 40), the gradient is a guarded
fp32 window and the workspace a guarded run of exactly the floats the launch owns (nslice * nprob * n * ntaps * c).  After every
launch: no store outside the gradient window or the workspace, no NaN in either - a read beside an operand's window or past its
last row, a DMA of a non-live ring slot that fetched something, an unwritten element all show.

Shapes are the smallest at which each branch of the slice arithmetic, the XCD remap and the combine kernels is live (tests/_dw_ref.py
holds the case tables): m = 64 (one pass of each wave group's loop), unit counts the slice count does not divide, slices that begin
inside a sample, hw_out = 1024, workgroup counts that are no multiple of 8, the clamp and the shrink of nslice, gradient rows on and
off the 16-byte grid, c = 160 (the short last block of wd_dw_combine_kernel), grouped launches with ntaps 1 and 9.

The reference is tests/_dw_ref.py (gated by tests/test_dw_ref_host.py) on the plane-rounded operands.  Bounds: the norm bounds of
tests/test_gpu_backward.py (5e-6 against the rounded operands, 2e-5 against the unrounded ones and on got - base under accumulate)
and, element by element, |got - ref| <= dw_beta(m, nslice) * S (+ 2^-24 |result| under accumulate), S = sum |d| |x|.  A grouped
launch must equal wd_dw alone on each item bit for bit: the per-(tile, slice) work and the ascending slice sum are the same code.

Measured on an MI355X, largest |got - ref| / S: linear 2.2e-6, 3x3 2.0e-6, grouped 2.6e-6 with three passes (the dropped lo.lo term,
below its 2^-18 = 3.8e-6) and 1e-7 with one pass, against a beta of 2.7e-5 (m = 64) to 3.7e-4 (m = 1024); each case prints its own."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _dw_ref as R  # noqa: E402
from tests import _guard as G  # noqa: E402
from tests._common import rel_err  # noqa: E402
from worddiffusion_amd import _native as N  # noqa: E402

DEV = "cuda:0"
F32 = torch.float32
EPS24 = 2.0 ** -24
NOTHING = (0, 0, 0, 0)  # the empty window: a buffer no launch may touch


def _st():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(got, want, name):
    bad = _bits(got) != _bits(want)
    assert not bool(bad.any()), (f"{name}: {int(bad.sum())} element(s) differ, first at {tuple(int(i) for i in bad.nonzero()[0])}: "
                                 f"{got.cpu()[tuple(bad.nonzero()[0])].item()!r} != {want.cpu()[tuple(bad.nonzero()[0])].item()!r}")


class _Operands:
    """The planes of one layer on the device: d [m][n] at column d_col of pitch d_ld, x [rows][c] at column x_col of pitch x_ld."""

    def __init__(self, d, x, d_extra=24, d_col=8, x_extra=40, x_col=16):
        self.d, self.x = d, x
        self.m, self.n = d.shape
        self.c = x.shape[1]
        self.db, self.dv = G.pitched_planes(d, self.n + d_extra, d_col, 2, DEV)
        self.xb, self.xv = G.pitched_planes(x, self.c + x_extra, x_col, 2, DEV)
        self.d_ld, self.x_ld = self.db.shape[-1], self.xb.shape[-1]
        for v, ld in ((self.dv, self.d_ld), (self.xv, self.x_ld)):
            assert ld % 8 == 0 and v[0].data_ptr() % 16 == 0 and v[1].data_ptr() % 16 == 0

    def fill(self, a, npass):
        """The operand fields of a wd_dw_args or a wd_dw_item."""
        a.d_hi, a.d_lo = self.dv[0].data_ptr(), (self.dv[1].data_ptr() if npass == 3 else None)
        a.x_hi, a.x_lo = self.xv[0].data_ptr(), (self.xv[1].data_ptr() if npass == 3 else None)
        a.d_ld, a.x_ld = self.d_ld, self.x_ld


class _Table:
    def __init__(self, tab):
        self.buf, self.view = G.pitched(torch.from_numpy(tab.reshape(1, -1).copy()), tab.size, 0, 2, DEV)


def _grad_window(n, kt, extra, col0, prior):
    """(buffer, window): the gradient [n][kt] at column col0 of pitch kt + extra; prior None: the window stays poisoned (accumulate 0
    must never read it), else what it holds before the launch."""
    buf, view = G.guarded(n, kt, kt + extra, col0, F32, 2, DEV)
    if prior is not None:
        view.copy_(prior)
    return buf, view


def _shape_args(m, n, c, ntaps, hw_out, hw_src, npass, nslice, table):
    a = N.WdDwArgs()
    a.m, a.n, a.c, a.ntaps, a.hw_out, a.hw_src, a.npass, a.nslice = m, n, c, ntaps, hw_out, hw_src, npass, nslice
    a.gather = table.view.data_ptr() if table is not None else None
    return a


def _check_buffers(grads, wsb, wsv, used):
    for i, (gb, gv) in enumerate(grads):
        G.assert_untouched(gb, gv, f"gradient {i}")
        G.assert_finite(gv, f"gradient {i}")
    G.assert_untouched(wsb, wsv, "workspace")
    G.assert_finite(wsv[:used], "workspace (the slabs of the launch)")


def _run_dw(ops, ntaps=1, table=None, hw_out=64, hw_src=64, npass=3, nslice=1, ws_slices=None, grad_extra=0, grad_col=0, prior=None):
    """One wd_dw launch behind guards.  ws_slices: slices the workspace holds (= the slices the launch must end up using; default
    nslice).  Returns the gradient window."""
    lib = N.lib()
    kt = ops.c * ntaps
    used = (ws_slices or nslice) * ops.n * kt
    gb, gv = _grad_window(ops.n, kt, grad_extra, grad_col, prior)
    wsb, wsv = G.guarded_flat(used, F32, 64, DEV)
    a = _shape_args(ops.m, ops.n, ops.c, ntaps, hw_out, hw_src, npass, nslice, table)
    ops.fill(a, npass)
    a.grad, a.grad_ld, a.accumulate = gv.data_ptr(), gb.shape[-1], int(prior is not None)
    a.ws, a.ws_floats = wsv.data_ptr(), used
    assert wsv.data_ptr() % 16 == 0
    N.check(lib.wd_dw(C.byref(a), _st()), "wd_dw")
    torch.cuda.synchronize()
    _check_buffers([(gb, gv)], wsb, wsv, used)
    return gv


_WORST = {}


def _check_result(family, name, got, d, x, npass, nslice, prior, ntaps=1, tab=None, hw_out=0, hw_src=0):
    """got against the specification: the project's norm bounds and the element-wise bound beta * S."""
    m = d.shape[0]
    ref, S = R.dw_ref(R.rounded(d, npass), R.rounded(x, npass), ntaps, tab, hw_out, hw_src)
    got = got.detach().cpu().double()
    beta = R.dw_beta(m, nslice)
    if prior is None:
        total, bound = ref, beta * S
        assert rel_err(got, ref) < 5e-6, name
    else:
        total = prior.double() + ref
        bound = beta * S + EPS24 * total.abs()
        assert rel_err(got - prior.double(), ref) < 2e-5, name
    if npass == 3:
        assert rel_err(got - (0 if prior is None else prior.double()), R.dw_ref(d, x, ntaps, tab, hw_out, hw_src)[0]) < 2e-5, name
    err = (got - total).abs()
    ratio = float((err / S).max())
    _WORST[family] = max(_WORST.get(family, 0.0), ratio)
    print(f"{name}: largest |got - ref| / S = {ratio:.3e} (beta {beta:.3e}); largest so far of {family}: {_WORST[family]:.3e}")
    bad = ~(err <= bound)
    assert not bool(bad.any()), (f"{name}: {int(bad.sum())} element(s) outside beta * S, first at {tuple(int(i) for i in bad.nonzero()[0])}: "
                                 f"got {got[tuple(bad.nonzero()[0])].item()!r}, want {total[tuple(bad.nonzero()[0])].item()!r}")


def _prior(n, kt, acc, key):
    return torch.randn(n, kt, generator=torch.Generator().manual_seed(977 + key)) if acc else None


# ------------------------------------------------------------------------------------------ linear layers: one tap, no table
@pytest.mark.parametrize("case", sorted(R.LINEAR_CASES))
def test_linear_weight_gradient_behind_guards(case):
    m, n, c, nslice, extra, col0, acc, npass = R.LINEAR_CASES[case]
    d, x = R.linear_inputs(m, n, c)
    used = nslice or N.lib().wd_dw_slices(m, n, c, 1)  # nslice 0: the workspace holds exactly the automatic count
    assert 1 <= used <= m // 64
    prior = _prior(n, c, acc, m + n)
    got = _run_dw(_Operands(d, x), npass=npass, nslice=nslice, ws_slices=used, grad_extra=extra, grad_col=col0, prior=prior)
    assert (got.data_ptr() % 16 == 0 and got.stride(0) % 4 == 0) == (extra == 12)  # the float4 path / the scalar path of combine1
    _check_result("linear", case, got, d, x, npass, used, prior)


@pytest.mark.parametrize("m,asked,holds", [(128, 7, 2), (256, 4, 2)], ids=["more_slices_than_units", "workspace_of_two_slices"])
def test_slice_count_is_clamped_to_units_and_workspace(m, asked, holds):
    """nslice above the unit count, or above what the workspace holds, runs with fewer slices: nothing outside the workspace, and the
    bits of the launch that asks for that count."""
    n = c = 160
    d, x = R.linear_inputs(m, n, c, key=asked)
    ops = _Operands(d, x)
    got = _run_dw(ops, nslice=asked, ws_slices=holds, grad_extra=12, grad_col=4)
    want = _run_dw(ops, nslice=holds, grad_extra=12, grad_col=4)
    _same_bits(got, want, f"nslice {asked} against nslice {holds}")
    _check_result("linear", f"m{m}_asked_{asked}", got, d, x, 3, holds, None)


# ------------------------------------------------------------------------------------------ 3x3 layers: nine taps through a table
@pytest.mark.parametrize("case", sorted(R.CONV_CASES))
def test_conv_weight_gradient_behind_guards(case):
    mode, B, h, w, n, c, nslice, extra, col0, acc, npass = R.CONV_CASES[case]
    d, x, tab, hw_out, hw_src = R.conv_inputs(mode, B, h, w, n, c)
    assert int((tab < 0).sum()) > 0 and d.shape[0] == B * hw_out <= 1024
    prior = _prior(n, 9 * c, acc, B + h + c)
    got = _run_dw(_Operands(d, x), 9, _Table(tab), hw_out, hw_src, npass, nslice, grad_extra=extra, grad_col=col0, prior=prior)
    _check_result("3x3", case, got, d, x, npass, nslice, prior, 9, tab, hw_out, hw_src)


# ------------------------------------------------------------------------------------------ wd_dw_group
def _run_group(items, ntaps, table, hw, npass, nslice):
    """items: (operands, grad_extra, grad_col, prior) per layer.  One wd_dw_group launch behind guards -> the gradient windows."""
    lib = N.lib()
    o0 = items[0][0]
    kt, nitems = o0.c * ntaps, len(items)
    arr = (N.WdDwItem * nitems)()
    grads = []
    for i, (ops, extra, col0, prior) in enumerate(items):
        gb, gv = _grad_window(o0.n, kt, extra, col0, prior)
        ops.fill(arr[i], npass)
        arr[i].grad, arr[i].grad_ld, arr[i].accumulate = gv.data_ptr(), gb.shape[-1], int(prior is not None)
        grads.append((gb, gv))
    dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    used = nslice * nitems * o0.n * kt
    wsb, wsv = G.guarded_flat(used, F32, 64, DEV)
    a = _shape_args(o0.m, o0.n, o0.c, ntaps, hw, hw, npass, nslice, table)
    a.ws, a.ws_floats = wsv.data_ptr(), used
    N.check(lib.wd_dw_group(C.byref(a), C.cast(arr, C.c_void_p), dev.data_ptr(), nitems, _st()), "wd_dw_group")
    torch.cuda.synchronize()
    _check_buffers(grads, wsb, wsv, used)
    return [gv for _, gv in grads]


# per item: (d_ld - n, d column, x_ld - c, x column, gradient pitch extra, gradient column, accumulate); the gradient windows of
# one tap: on the 16-byte grid, off it, on it
_ITEM_DRESS = [(24, 8, 40, 16, 12, 4, 0), (32, 16, 56, 8, 13, 3, 1), (8, 0, 48, 24, 12, 0, 1)]


@pytest.mark.parametrize("ntaps,nitems,n,nslice,npass", R.GROUP_CASES)
def test_group_of_layers_equals_each_layer_alone(ntaps, nitems, n, nslice, npass):
    """The 4x16 map at batch 2 (m = 128, hw_out = hw_src = 64): the linear layers of a transformer block, or the two 3x3 convolutions
    of a ResBlock (ntaps 9, one gather table), in one launch - blockIdx.y > 0 in the combine kernels, a.items set in wd_dw_kernel."""
    mode, B, h, w = R.GROUP_MAP
    c, m, hw = n, B * h * w, h * w
    tab, table, items, inputs = None, None, [], []
    for i in range(nitems):
        de, dc, xe, xc, ge, gc, acc = _ITEM_DRESS[i]
        if ntaps == 9:
            d, x, tab, _, _ = R.conv_inputs(mode, B, h, w, n, c, key=i)
            table = table or _Table(tab)
            ge, gc = (5, 3) if i != 1 else (8, 4)
        else:
            d, x = R.linear_inputs(m, n, c, key=i)
        items.append((_Operands(d, x, de, dc, xe, xc), ge, gc, _prior(n, c * ntaps, acc, i)))
        inputs.append((d, x))
    got = _run_group(items, ntaps, table, hw, npass, nslice)
    for i, (ops, ge, gc, prior) in enumerate(items):
        alone = _run_dw(ops, ntaps, table, hw, hw, npass, nslice, grad_extra=ge, grad_col=gc, prior=prior)
        _same_bits(got[i], alone, f"item {i} of {nitems} against wd_dw alone")
        _check_result("group", f"taps{ntaps}_n{n}_item{i}of{nitems}", got[i], *inputs[i], npass, nslice, prior, ntaps, tab, hw, hw)


# ------------------------------------------------------------------------------------------ the contract
def _valid(ntaps=1, nprob=1):
    """A launch wd_dw accepts (m = 128, n = c = 160, hw 64, two slices of nprob layers) whose gradient and workspace are buffers NO
    launch may touch."""
    m, n, c, B, h, w = 128, 160, 160, 2, 4, 16
    if ntaps == 9:
        d, x, tab, _, _ = R.conv_inputs("same", B, h, w, n, c)
        table = _Table(tab)
    else:
        (d, x), table = R.linear_inputs(m, n, c), None
    ops = _Operands(d, x)
    gb = G.poisoned((n + 4, c * ntaps + 16), F32, DEV)
    wsb = G.poisoned((1, 2 * nprob * n * c * ntaps + 128), F32, DEV)
    a = _shape_args(m, n, c, ntaps, 64, 64, 3, 2, table)
    ops.fill(a, 3)
    a.grad, a.grad_ld, a.accumulate = gb[2:, 4:].data_ptr(), gb.shape[-1], 0
    a.ws, a.ws_floats = wsb[:, 64:].data_ptr(), 2 * nprob * n * c * ntaps
    return a, (ops, table, gb, wsb)


def _set(**kw):
    def f(a):
        for k, v in kw.items():
            setattr(a, k, v)
    return f


def _shift(field, nbytes):
    def f(a):
        setattr(a, field, getattr(a, field) + nbytes)
    return f


_REFUSED = {
    "d_ld_below_n": (1, _set(d_ld=152)),
    "x_ld_below_c": (1, _set(x_ld=152)),
    "d_ld_no_multiple_of_8": (1, _set(d_ld=188)),
    "x_ld_no_multiple_of_8": (1, _set(x_ld=204)),
    "d_hi_8_bytes_off": (1, _shift("d_hi", 8)),
    "x_lo_8_bytes_off": (1, _shift("x_lo", 8)),
    "grad_ld_below_c": (1, _set(grad_ld=159)),
    "grad_ld_below_9c": (9, _set(grad_ld=9 * 160 - 1)),
    "npass_2": (1, _set(npass=2)),
    "npass_3_without_d_lo": (1, _set(d_lo=None)),
    "npass_3_without_x_lo": (1, _set(x_lo=None)),
    "ws_null": (1, _set(ws=None)),
    "ws_4_bytes_off": (1, _shift("ws", 4)),
    "ws_below_one_slice": (1, _set(ws_floats=160 * 160 - 1)),
    "nine_taps_without_table": (9, _set(gather=None)),
    "no_table_and_hw_src_differs": (1, _set(hw_src=256)),
    "table_and_hw_src_0": (9, _set(hw_src=0)),
    "hw_out_1088": (1, _set(m=1088, hw_out=1088, hw_src=1088)),
    "m_96": (1, _set(m=96)),
    # sizes only: the planes these would need do not exist, the check is made on the host before any launch
    "d_planes_of_2_GiB": (1, _set(m=1024, d_ld=1 << 20)),
    "x_planes_of_2_GiB": (1, _set(m=1024, x_ld=1 << 20)),
}


@pytest.mark.parametrize("ntaps,nitems", [(1, 0), (9, 0), (1, 3)])
def test_the_launch_the_refusals_start_from_is_accepted(ntaps, nitems):
    """Unchanged, the arguments of _valid / _valid_group run: each refusal below is owed to the one field it changes."""
    lib = N.lib()
    if nitems:
        a, arr, (ops, table, gb, wsb) = _valid_group(nitems)
        dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
        N.check(lib.wd_dw_group(C.byref(a), C.cast(arr, C.c_void_p), dev.data_ptr(), nitems, _st()), "wd_dw_group")
    else:
        a, (ops, table, gb, wsb) = _valid(ntaps)
        N.check(lib.wd_dw(C.byref(a), _st()), "wd_dw")
    torch.cuda.synchronize()
    G.assert_untouched(gb, (2, 160, 4, 160 * ntaps), "gradient")
    G.assert_untouched(wsb, (0, 1, 64, int(a.ws_floats)), "workspace")
    G.assert_finite(gb[2:162, 4:4 + 160 * ntaps], "gradient")


@pytest.mark.parametrize("case", sorted(_REFUSED))
def test_dw_refuses(case):
    ntaps, change = _REFUSED[case]
    a, (ops, table, gb, wsb) = _valid(ntaps)
    change(a)
    assert N.lib().wd_dw(C.byref(a), _st()) == N.WD_EINVAL
    torch.cuda.synchronize()
    G.assert_untouched(gb, NOTHING, "gradient of a refused launch")
    G.assert_untouched(wsb, NOTHING, "workspace of a refused launch")


def _valid_group(nitems):
    """nitems good items (the same layer nitems times) and a workspace that holds them: the named fault is the only reason to refuse."""
    a, keep = _valid(1, nitems)
    arr = (N.WdDwItem * nitems)()
    for it in arr:
        for f in ("d_hi", "d_lo", "x_hi", "x_lo", "grad", "d_ld", "x_ld", "grad_ld", "accumulate"):
            setattr(it, f, getattr(a, f))
    return a, arr, keep


@pytest.mark.parametrize("case", ["no_items", "65_items", "null_host_table", "null_device_table", "one_bad_item"])
def test_dw_group_refuses(case):
    lib = N.lib()
    nitems = {"no_items": 0, "65_items": 65}.get(case, 3)
    a, arr, (ops, table, gb, wsb) = _valid_group(max(nitems, 1))
    if case == "one_bad_item":
        arr[1].x_ld = 152
    dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    host = None if case == "null_host_table" else C.cast(arr, C.c_void_p)
    assert lib.wd_dw_group(C.byref(a), host, None if case == "null_device_table" else dev.data_ptr(), nitems, _st()) == N.WD_EINVAL
    torch.cuda.synchronize()
    G.assert_untouched(gb, NOTHING, "gradient of a refused launch")
    G.assert_untouched(wsb, NOTHING, "workspace of a refused launch")
