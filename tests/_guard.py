"""Guard bands and poison for the kernel tests: an operand is a window of a wider, taller buffer whose every other element holds
a fixed NaN bit pattern.  A store outside the window changes the pattern (assert_untouched names the first element); a read
outside it brings a NaN into the window (assert_finite names the first).  Plain functions, no fixtures."""
import torch

NAN32 = 0x7FFBADAD  # a NaN as fp32 and as the high half of an fp64 (both halves of a double get it); no arithmetic produces it
NAN16 = 0x7FD5      # a bf16 NaN
_INT = {torch.float32: (torch.int32, 1, NAN32), torch.int32: (torch.int32, 1, NAN32), torch.float64: (torch.int32, 2, NAN32),
        torch.bfloat16: (torch.int16, 1, NAN16)}


def _ints(t):
    """t's bits as integers [..., rows, ld * k] (k = integers per element), and the fill pattern."""
    it, k, pat = _INT[t.dtype]
    return (t if t.dtype == it else t.view(it)), k, pat


def poisoned(shape, dtype, device="cpu"):
    it, k, pat = _INT[dtype]
    shape = tuple(shape)
    raw = torch.full(shape[:-1] + (shape[-1] * k,), pat, dtype=it, device=device)
    return raw if dtype == it else raw.view(dtype)


def guarded(rows, cols, ld, col0, dtype, guard_rows=2, device="cpu", planes=0):
    """(buf, view): buf has rows + 2 * guard_rows rows of pitch ld, every element the NaN pattern; view is the rows x cols window
    at row guard_rows, column col0.  planes = 2: two such buffers stacked (the hi / lo planes), view [2][rows][cols]."""
    assert 0 <= col0 and col0 + cols <= ld and guard_rows >= 0
    lead = (planes,) if planes else ()
    buf = poisoned(lead + (rows + 2 * guard_rows, ld), dtype, device)
    return buf, buf[..., guard_rows:guard_rows + rows, col0:col0 + cols]


def guarded_flat(n, dtype, pad=64, device="cpu"):
    """(buf, view): a contiguous run of n elements - a scratch buffer, a [b][chunk][2][c] block of sums, any output that has no pitch
    of its own - with pad poisoned elements before and after it.  buf is [1][n + 2 * pad], view its 1-D window of n elements
    (pad = 64 keeps a 16-byte aligned buffer's window 16-byte aligned for every element type)."""
    buf, view = guarded(1, n, n + 2 * pad, pad, dtype, 0, device)
    return buf, view[0]


def pitched(x, ld, col0, guard_rows=2, device="cpu"):
    """The 2-D tensor x placed as guarded() places a window, NaN everywhere else."""
    buf, view = guarded(x.shape[0], x.shape[1], ld, col0, x.dtype, guard_rows, device)
    view.copy_(x)
    return buf, view


def split_planes(x):
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return torch.stack([hi, lo], 0)


def pitched_planes(x, ld, col0, guard_rows=2, device="cpu"):
    """The split-bf16 planes of x ([2][rows][c]: hi = bf16(x), lo = bf16(x - hi)) placed the same way, bf16 NaN outside."""
    buf, view = guarded(x.shape[0], x.shape[1], ld, col0, torch.bfloat16, guard_rows, device, planes=2)
    view.copy_(split_planes(x.float()))
    return buf, view


def view_spec(buf, view):
    """(row0, rows, col0, cols) of a window made by guarded() inside its buffer."""
    ld = buf.shape[-1]
    off = view.storage_offset() - buf.storage_offset()
    off %= buf.shape[-2] * ld  # (the same window in every plane)
    return off // ld, (view.shape[-2] if view.dim() > 1 else 1), off % ld, view.shape[-1]  # (1-D: the window of guarded_flat)


def assert_untouched(buf, spec, name="buffer"):
    """Everything of buf outside the window still holds the fill pattern, compared as integers.  spec: the view guarded()
    returned, or (row0, rows, col0, cols)."""
    row0, rows, col0, cols = view_spec(buf, spec) if torch.is_tensor(spec) else spec
    ints, k, pat = _ints(buf.detach().cpu())
    bad = ints != pat
    bad[..., row0:row0 + rows, col0 * k:(col0 + cols) * k] = False
    if bool(bad.any()):
        idx = [int(v) for v in bad.nonzero()[0]]
        r, c = idx[-2], idx[-1] // k
        where = f"plane {idx[0]}, " if len(idx) == 3 else ""
        val = buf[tuple(idx[:-2]) + (r, c)].item()
        raise AssertionError(f"{name}: write outside the {rows} x {cols} window at (row {row0}, column {col0}): {int(bad.sum())} "
                             f"element(s), first at {where}(row {r}, column {c}) = {val!r}")


def row_windows(batch, stride, row0, rows, col0, cols):
    """One window per sample, as the attention kernels place their output: rows b * stride + row0 .. + rows, columns col0 .. + cols."""
    return [(b * stride + row0, rows, col0, cols) for b in range(batch)]


def assert_untouched_windows(buf, windows, name="buffer"):
    """assert_untouched for an output that is several windows of one buffer: everything outside ALL of them still holds the fill
    pattern.  windows: a list of (row0, rows, col0, cols), or a boolean keep-mask over buf's last two dimensions (True = may
    change; the same in every plane)."""
    ints, k, pat = _ints(buf.detach().cpu())
    if torch.is_tensor(windows):
        assert windows.dtype == torch.bool and tuple(windows.shape) == tuple(buf.shape[-2:]), "keep-mask: bool [rows][ld]"
        keep, what = windows.cpu(), f"the {int(windows.sum())} kept element(s)"
    else:
        keep = torch.zeros(buf.shape[-2:], dtype=torch.bool)
        for row0, rows, col0, cols in windows:
            assert 0 <= row0 and row0 + rows <= buf.shape[-2] and 0 <= col0 and col0 + cols <= buf.shape[-1], "window outside buf"
            keep[row0:row0 + rows, col0:col0 + cols] = True
        what = f"the {len(windows)} window(s)" + (f" of {windows[0][1]} x {windows[0][3]}, first at (row {windows[0][0]}, column "
                                                  f"{windows[0][2]})" if windows else "")
    bad = (ints != pat) & ~keep.repeat_interleave(k, dim=-1)
    if bool(bad.any()):
        idx = [int(v) for v in bad.nonzero()[0]]
        r, c = idx[-2], idx[-1] // k
        where = f"plane {idx[0]}, " if len(idx) == 3 else ""
        val = buf[tuple(idx[:-2]) + (r, c)].item()
        raise AssertionError(f"{name}: write outside {what}: {int(bad.sum())} element(s), first at {where}(row {r}, column {c}) "
                             f"= {val!r}")


def assert_finite(view, name="window"):
    """Every window value is finite (an unwritten element or a poisoned operand read shows as NaN)."""
    v = view.detach().float().cpu() if view.dtype == torch.bfloat16 else view.detach().cpu()
    bad = ~torch.isfinite(v)
    if bool(bad.any()):
        idx = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError(f"{name}: {int(bad.sum())} non-finite value(s), first at {idx} = {v[idx].item()!r}")
