"""The guard-band helper of the pitched-operand kernel tests (tests/_guard.py) can fail: one element written into the padding and
one NaN put into a window are both reported, with their position, for every element type the kernels write.  No GPU."""
import pytest
import torch

from tests import _guard as G


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16, torch.int32])
@pytest.mark.parametrize("planes", [0, 2])
def test_guard_bands_report_a_write_outside_the_window(dtype, planes):
    buf, view = G.guarded(5, 6, 12, 4, dtype, planes=planes)
    assert buf.shape[-2:] == (9, 12) and view.shape[-2:] == (5, 6) and G.view_spec(buf, view) == (2, 5, 4, 6)
    if dtype.is_floating_point:
        assert bool(torch.isnan(buf.float()).all())  # the fill is a NaN in every type
    G.assert_untouched(buf, view)
    view.fill_(1)  # the whole window may change
    G.assert_untouched(buf, view)
    G.assert_untouched(buf, (2, 5, 4, 6))
    for r, c in [(2, 3), (2, 10), (1, 4), (7, 9), (0, 0), (8, 11), (4, 0)]:  # left / right padding, rows before / after, corners
        b2 = buf.clone()
        b2[..., r, c] = 3
        with pytest.raises(AssertionError, match=rf"\(row {r}, column {c}\) = 3"):
            G.assert_untouched(b2, (2, 5, 4, 6), "out")
    if planes:
        b2 = buf.clone()
        b2[1, 6, 11] = 0
        with pytest.raises(AssertionError, match=r"plane 1, \(row 6, column 11\)"):
            G.assert_untouched(b2, view)


def test_guard_sees_half_a_double_change():
    buf, view = G.guarded(2, 2, 4, 1, torch.float64)
    ints = buf.view(torch.int32)
    ints[3, 7] = 0  # the high half of (row 3, column 3)
    with pytest.raises(AssertionError, match=r"\(row 3, column 3\)"):
        G.assert_untouched(buf, view)


def test_poisoned_operands_and_the_finite_check():
    x = torch.arange(12, dtype=torch.float32).reshape(3, 4) * (1 + 2.0 ** -12)  # hi = k, lo = k / 4096: exact
    buf, view = G.pitched(x, 8, 4)
    assert torch.equal(view, x) and int(torch.isnan(buf).sum()) == buf.numel() - 12
    G.assert_untouched(buf, view)
    G.assert_finite(view)
    pbuf, pview = G.pitched_planes(x, 16, 8)
    assert pbuf.shape == (2, 7, 16) and pbuf.dtype == torch.bfloat16
    assert torch.equal(pview[0].float() + pview[1].float(), x)
    assert int(torch.isnan(pbuf.float()).sum()) == pbuf.numel() - 24
    G.assert_untouched(pbuf, pview)
    G.assert_finite(pview)
    view[1, 2] = float("nan")
    with pytest.raises(AssertionError, match=r"first at \(1, 2\)"):
        G.assert_finite(view, "out")
    pview[1, 0, 3] = float("inf")
    with pytest.raises(AssertionError, match=r"first at \(1, 0, 3\)"):
        G.assert_finite(pview)
    # a value computed from a poisoned element is itself caught
    out, oview = G.guarded(3, 4, 4, 0, torch.float32, guard_rows=0)
    buf, view = G.pitched(x, 8, 4)
    oview.copy_(buf[2:5, 3:7] + 1)  # a window read one column too far to the left
    with pytest.raises(AssertionError, match=r"3 non-finite"):
        G.assert_finite(oview)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16])
def test_flat_guard_reports_a_write_before_and_after_the_run(dtype):
    """guarded_flat: the contiguous outputs of the backward kernels (scratch, [b][chunk][2][c] sums, [b][nwg][nk][2][inner] partials)."""
    buf, view = G.guarded_flat(2 * 3 * 2 * 8, dtype, pad=16)
    assert buf.shape == (1, 96 + 32) and view.shape == (96,) and view.is_contiguous() and G.view_spec(buf, view) == (0, 1, 16, 96)
    assert view.data_ptr() - buf.data_ptr() == 16 * buf.element_size()
    assert bool(torch.isnan(buf.float()).all())
    G.assert_untouched(buf, view)
    view.view(2, 3, 2, 8).fill_(1)  # the kernels' own shape over the same storage
    G.assert_untouched(buf, view)
    G.assert_finite(view.view(2, 3, 2, 8))
    for c in (15, 112, 0, 127):  # the element before the run, the one after it, the two ends of the buffer
        b2 = buf.clone()
        b2[0, c] = 3
        with pytest.raises(AssertionError, match=rf"\(row 0, column {c}\) = 3"):
            G.assert_untouched(b2, (0, 1, 16, 96), "sums")
    view[95] = float("nan")
    with pytest.raises(AssertionError, match=r"first at \(1, 2, 1, 7\)"):
        G.assert_finite(view.view(2, 3, 2, 8))


def test_a_window_as_wide_as_its_buffer_is_guarded_by_rows_alone():
    """The transposed planes [n][mpad] have no pitch of their own: a row of the next channel (or a row past the last) is the guard,
    and an empty window (a launch that must not happen) makes every element one."""
    buf, view = G.guarded(3, 8, 8, 0, torch.bfloat16, guard_rows=1, planes=2)
    view.fill_(0)
    G.assert_untouched(buf, view)
    for r in (0, 4):
        b2 = buf.clone()
        b2[1, r, 2] = 0
        with pytest.raises(AssertionError, match=rf"plane 1, \(row {r}, column 2\)"):
            G.assert_untouched(b2, view)
    with pytest.raises(AssertionError, match=r"24 element\(s\), first at plane 0, \(row 1, column 0\)"):
        G.assert_untouched(buf[:1], (0, 0, 0, 0))
    G.assert_untouched(G.poisoned((2, 5, 8), torch.bfloat16), (0, 0, 0, 0))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16])
@pytest.mark.parametrize("planes", [0, 2])
def test_several_windows_report_a_write_between_them(dtype, planes):
    """assert_untouched_windows: the attention output - one window of nq rows per sample at rows b * out_rows + out_row0 of one
    pitched buffer - as a list of windows and as a keep-mask; a write into the rows between two samples' windows, beside a window
    and past the last one is named by its position."""
    B, nq, out_rows, row0, cols, ld, col0 = 3, 4, 7, 2, 6, 12, 4
    lead = (planes,) if planes else ()
    buf = G.poisoned(lead + (B * out_rows, ld), dtype)
    wins = G.row_windows(B, out_rows, row0, nq, col0, cols)
    assert wins == [(2, 4, 4, 6), (9, 4, 4, 6), (16, 4, 4, 6)]
    mask = torch.zeros(B * out_rows, ld, dtype=torch.bool)
    for r0, nr, c0, nc in wins:
        mask[r0:r0 + nr, c0:c0 + nc] = True
    G.assert_untouched_windows(buf, wins)
    G.assert_untouched_windows(buf, mask)
    for r0, nr, c0, nc in wins:  # every window may change, whole
        buf[..., r0:r0 + nr, c0:c0 + nc] = 1
    G.assert_untouched_windows(buf, wins)
    G.assert_untouched_windows(buf, mask)
    # the row after a sample's last query, the rows before the next sample's first, beside a window, the ends of the buffer
    for r, c in [(6, 4), (7, 9), (8, 4), (13, 5), (9, 3), (12, 10), (0, 0), (20, 9), (20, 11)]:
        b2 = buf.clone()
        b2[..., r, c] = 3
        for w in (wins, mask):
            with pytest.raises(AssertionError, match=rf"out: write outside .*first at (plane 0, )?\(row {r}, column {c}\) = 3"):
                G.assert_untouched_windows(b2, w, "out")
    b2 = buf.clone()
    b2[..., 6, 4] = 3
    b2[..., 13, 4] = 3
    with pytest.raises(AssertionError, match=r"element\(s\), first at (plane 0, )?\(row 6, column 4\)"):  # the first of the two
        G.assert_untouched_windows(b2, wins)
    if planes:
        b2 = buf.clone()
        b2[1, 15, 11] = 0
        with pytest.raises(AssertionError, match=r"plane 1, \(row 15, column 11\)"):
            G.assert_untouched_windows(b2, wins)
    # one window: the same verdict as assert_untouched; no window: every element is guarded
    G.assert_untouched_windows(G.poisoned((5, 8), dtype), [])
    one = buf.clone()
    with pytest.raises(AssertionError, match=r"first at (plane 0, )?\(row 9, column 4\)"):
        G.assert_untouched_windows(one, wins[:1])
    with pytest.raises(AssertionError, match=r"first at (plane 0, )?\(row 9, column 4\)"):
        G.assert_untouched(one, wins[0])


def test_several_windows_see_half_a_double_and_reject_a_bad_mask():
    buf = G.poisoned((6, 4), torch.float64)
    wins = [(0, 2, 1, 2), (3, 2, 1, 2)]
    buf.view(torch.int32)[2, 3] = 0  # the high half of (row 2, column 1): between the windows
    with pytest.raises(AssertionError, match=r"\(row 2, column 1\)"):
        G.assert_untouched_windows(buf, wins)
    with pytest.raises(AssertionError, match="keep-mask"):
        G.assert_untouched_windows(buf, torch.zeros(6, 8, dtype=torch.bool))
    with pytest.raises(AssertionError, match="window outside buf"):
        G.assert_untouched_windows(buf, [(4, 3, 0, 1)])
