"""The two kernels of writer-free guidance and the contract of ``wd_embedding_bwd`` they lean on, on windows of NaN-filled buffers
(``tests/_guard.py``): nothing outside a window may be written, nothing outside an operand read.

  wd_label_rows_keep   mask, ``y_eff`` and ``keep_out`` equal the host specification (``tests/_labeldrop_ref.py``) exactly, kept rows
                       are ``label[y]`` bit for bit, dropped rows are all-zero bits; the host row base and the device-read one
                       agree; two launches of B rows at consecutive bases are one launch of 2B rows.
  wd_emb_combine_keep  kept rows are ``wd_emb_combine``'s bits, dropped rows those of ``wd_emb_combine`` on an all-zero table;
                       against float64 the bar of ``test_emb_combine_mix_kernel``: 2^-16 |v| + 1e-6 per element.
  wd_embedding_bwd     rows whose id is -1 or ``vocab`` contribute nothing: bit for bit the run on the remaining rows."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _guard as G  # noqa: E402
from tests import _labeldrop_ref as R  # noqa: E402
from worddiffusion_amd import _native as N  # noqa: E402
from worddiffusion_amd import dropout as DO  # noqa: E402

DEV = "cuda:0"
NCLS = 339


def _st():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def drop_args(seed, p, row_base, row_dev=None):
    d = DO.WdDropout()
    d.seed, d.row_base, d.row_base_dev = seed, row_base, None if row_dev is None else row_dev.data_ptr()
    d.tag, d.thr, d.scale = R.label_tag(), R.threshold(p), 123.0  # (scale is ignored)
    return d


def guarded_bytes(n, dtype):
    """(buf, view): ``n`` elements of an 8- or 1-byte integer type as a window of a NaN-patterned int32 buffer; the window is
    rounded up to whole int32 words, whose spare bytes must keep the pattern too (``spare_untouched``)."""
    size = torch.empty((), dtype=dtype).element_size()
    words = (n * size + 3) // 4
    buf, view = G.guarded_flat(words, torch.int32, device=DEV)
    return buf, view, view.view(dtype)[:n]


def spare_untouched(view, n, dtype):
    raw = view.cpu().view(torch.uint8)
    size = torch.empty((), dtype=dtype).element_size()
    pat = torch.tensor([G.NAN32], dtype=torch.int32).view(torch.uint8).repeat(view.numel())
    return torch.equal(raw[n * size:], pat[n * size:])


def label_table(ted, seed):
    g = torch.Generator().manual_seed(seed)
    label = torch.randn(NCLS, ted, generator=g)
    lbuf, lview = G.guarded_flat(NCLS * ted, torch.float32, device=DEV)
    lview.copy_(label.reshape(-1))
    return label, lbuf, lview


def run_label_rows(lib, lview, y, ted, d=None, keep_in=None):
    """One launch into fresh guarded outputs -> (out [B, ted], y_eff [B], keep_out [B]) on the host, after the guard checks."""
    B = y.numel()
    ybuf, yraw, yv = guarded_bytes(B, torch.int64)
    yv.copy_(y)
    obuf, oview = G.guarded_flat(B * ted, torch.float32, device=DEV)
    ebuf, eraw, ev = guarded_bytes(B, torch.int64)
    kbuf, kraw, kv = guarded_bytes(B, torch.uint8)
    kin = None
    if keep_in is not None:
        ibuf, iraw, kin = guarded_bytes(B, torch.uint8)
        kin.copy_(keep_in)
    N.check(lib.wd_label_rows_keep(lview.data_ptr(), yv.data_ptr(), NCLS, B, ted, None if d is None else C.byref(d),
                                   None if kin is None else kin.data_ptr(), oview.data_ptr(), ev.data_ptr(), kv.data_ptr(), _st()),
            "wd_label_rows_keep")
    torch.cuda.synchronize()
    for name, buf, view in (("out", obuf, oview), ("y_eff", ebuf, eraw), ("keep_out", kbuf, kraw), ("y", ybuf, yraw)):
        G.assert_untouched(buf, view, name)
    assert spare_untouched(kraw, B, torch.uint8), "keep_out: a byte past the B decisions was written"
    assert torch.equal(yv.cpu(), y), "y was written"
    G.assert_finite(oview, "out")  # (a read outside the label table would bring its NaN in)
    return oview.cpu().reshape(B, ted), ev.cpu(), kv.cpu()


def check_rows(out, y_eff, keep_out, label, y, keep, what):
    keep_t = torch.from_numpy(np.asarray(keep, dtype=bool))
    assert torch.equal(keep_out, keep_t.to(torch.uint8)), (what, keep_out.tolist(), keep_t.tolist())
    assert torch.equal(y_eff, torch.from_numpy(R.y_eff(y.numpy(), keep_t.numpy()))), what
    assert torch.equal(out[keep_t], label[y[keep_t]]), f"{what}: a kept row is not label[y] bit for bit"
    assert not bool(out[~keep_t].view(torch.int32).any()), f"{what}: a dropped row is not all-zero bits"


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("B,ted", [(5, 256), (3, 1280)])
def test_label_rows_keep(B, ted, p):
    lib = N.lib()
    seed, row_base, _, _ = R.DRAWS[f"kernel B={B} p={p}"]
    assert R.DRAWS[f"kernel B={B} p={p}, next rows"] == (seed, row_base + B, B, p)
    label, lbuf, lview = label_table(ted, B + ted)
    g = torch.Generator().manual_seed(int(p * 10) + B)
    y2 = torch.randint(0, NCLS, (2 * B,), generator=g)
    y2[0], y2[B - 1] = NCLS - 1, 0  # the ends of the table
    y = y2[:B]
    keep = R.keep_mask(seed, row_base, B, p)
    # the whole row base in the struct / split between the struct and the device word
    host = run_label_rows(lib, lview, y, ted, d=drop_args(seed, p, row_base))
    check_rows(*host, label, y, keep, "host row base")
    row_dev = torch.tensor([2], dtype=torch.int64, device=DEV)
    dev = run_label_rows(lib, lview, y, ted, d=drop_args(seed, p, row_base - 2, row_dev))
    check_rows(*dev, label, y, keep, "device-read row base")
    assert all(torch.equal(a, b) for a, b in zip(host, dev))
    # two launches of B rows at consecutive bases == one launch of 2B rows
    nxt = run_label_rows(lib, lview, y2[B:], ted, d=drop_args(seed, p, row_base + B))
    both = run_label_rows(lib, lview, y2, ted, d=drop_args(seed, p, row_base))
    check_rows(*both, label, y2, R.keep_mask(seed, row_base, 2 * B, p), "2B rows")
    for a, b, c in zip(host, nxt, both):
        assert torch.equal(torch.cat([a, b]), c)
    # an explicit mask instead of the draw (any nonzero byte keeps)
    given = torch.tensor([1, 0, 7, 1, 0][:B], dtype=torch.uint8)
    exp = run_label_rows(lib, lview, y, ted, keep_in=given)
    check_rows(*exp, label, y, given.numpy() != 0, "keep_in")
    # the draw wins over keep_in when both are handed in (d != NULL)
    drawn = run_label_rows(lib, lview, y, ted, d=drop_args(seed, p, row_base), keep_in=given)
    assert all(torch.equal(a, b) for a, b in zip(host, drawn))
    G.assert_untouched(lbuf, lview, "label")


def test_label_rows_keep_rows_past_2_32_and_bad_arguments():
    lib = N.lib()
    seed, row_base, B, p = R.DRAWS["kernel rows past 2^32"]
    ted = 256
    label, lbuf, lview = label_table(ted, 9)
    y = torch.tensor([5, 338, 0, 17, 200])
    keep = R.keep_mask(seed, row_base, B, p)
    assert not np.array_equal(keep, R.keep_mask(seed, row_base & 0xFFFFFFFF, B, p))  # the high word of the row is in the counter
    row_dev = torch.tensor([1 << 32], dtype=torch.int64, device=DEV)
    got = run_label_rows(lib, lview, y, ted, d=drop_args(seed, p, row_base - (1 << 32), row_dev))
    check_rows(*got, label, y, keep, "rows past 2^32")
    # y_eff / keep_out are optional
    yd = y.to(DEV)
    out = torch.full((B, ted), float("nan"), device=DEV)
    d = drop_args(seed, p, row_base)
    N.check(lib.wd_label_rows_keep(lview.data_ptr(), yd.data_ptr(), NCLS, B, ted, C.byref(d), None, out.data_ptr(), None, None, _st()),
            "wd_label_rows_keep")
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), got[0])
    # refused, nothing launched: neither a draw nor a mask; ted % 4; a NULL output
    out.fill_(float("nan"))
    kin = torch.ones(B, dtype=torch.uint8, device=DEV)
    assert lib.wd_label_rows_keep(lview.data_ptr(), yd.data_ptr(), NCLS, B, ted, None, None, out.data_ptr(), None, None, _st()) == N.WD_EINVAL
    assert lib.wd_label_rows_keep(lview.data_ptr(), yd.data_ptr(), NCLS, B, 254, None, kin.data_ptr(), out.data_ptr(), None, None,
                                  _st()) == N.WD_EINVAL
    assert lib.wd_label_rows_keep(lview.data_ptr(), yd.data_ptr(), NCLS, B, ted, None, kin.data_ptr(), None, None, None, _st()) == N.WD_EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


def _planes_value(pl):
    return pl[0].float().double() + pl[1].float().double()


def test_emb_combine_keep_kernel():
    lib = N.lib()
    T, B, ted = 19, 5, 256  # ragged batch; 19 timesteps in two calls of 10 and 9 rows of ``time``, as the engine's chunks
    g = torch.Generator().manual_seed(3)
    time = torch.randn(T, ted, generator=g)
    assert not bool((time == 0).any())
    label = torch.randn(NCLS, ted, generator=g)
    y = torch.tensor([338, 0, 17, 200, 5])
    keep = torch.tensor([1, 0, 1, 1, 0], dtype=torch.uint8)
    tbuf, tview = G.pitched(time, ted, 0, device=DEV)  # (contiguous rows: the kernel takes no pitch for ``time``)
    lbuf, lview = G.guarded_flat(NCLS * ted, torch.float32, device=DEV)
    lview.copy_(label.reshape(-1))
    yd, kd = y.to(DEV), keep.to(DEV)
    zero = torch.zeros(NCLS, ted, device=DEV)

    def plain(table):
        pl = torch.zeros(2, T * B, ted, dtype=torch.bfloat16, device=DEV)
        N.check(lib.wd_emb_combine(tview.data_ptr(), table, yd.data_ptr(), NCLS, T, B, ted, pl[0].data_ptr(), pl[1].data_ptr(), ted,
                                   _st()), "wd_emb_combine")
        torch.cuda.synchronize()
        return pl.cpu().view(torch.int16).reshape(2, T, B, ted)

    with_label, without = plain(lview.data_ptr()), plain(zero.data_ptr())

    def keep_run(keep_ptr, lab_ptr, y_ptr, ncls):
        ld, col0 = ted + 16, 8
        buf, view = G.guarded(T * B, ted, ld, col0, torch.bfloat16, device=DEV, planes=2)
        for t0, nt in ((0, 10), (10, 9)):
            N.check(lib.wd_emb_combine_keep(tview[t0].data_ptr(), lab_ptr, y_ptr, keep_ptr, ncls, nt, B, ted,
                                            view[0, t0 * B].data_ptr(), view[1, t0 * B].data_ptr(), ld, _st()), "wd_emb_combine_keep")
        torch.cuda.synchronize()
        G.assert_untouched(buf, view, "planes")
        G.assert_finite(view, "planes")
        return view.cpu().contiguous()

    got = keep_run(kd.data_ptr(), lview.data_ptr(), yd.data_ptr(), NCLS)
    bits = got.view(torch.int16).reshape(2, T, B, ted)
    kb = keep.bool()
    assert torch.equal(bits[:, :, kb], with_label[:, :, kb]), "a kept row is not wd_emb_combine's, bit for bit"
    assert torch.equal(bits[:, :, ~kb], without[:, :, ~kb]), "a dropped row is not wd_emb_combine's on a zero table, bit for bit"
    assert not torch.equal(with_label[:, :, ~kb], without[:, :, ~kb])
    lab64 = label.double()[y] * kb.double()[:, None]
    ref = torch.nn.functional.silu(time.double()[:, None, :] + lab64[None]).reshape(T * B, ted)
    err = (_planes_value(got) - ref).abs()
    print(f"wd_emb_combine_keep: max |err| / (|v| + 1) = {float((err / (ref.abs() + 1)).max()):.3e}")
    assert (err <= 2.0 ** -16 * ref.abs() + 1e-6).all()
    # keep == NULL: no sample keeps its writer; label and y may be NULL
    for lab_ptr, y_ptr, ncls in ((None, None, 0), (lview.data_ptr(), yd.data_ptr(), NCLS)):
        none = keep_run(None, lab_ptr, y_ptr, ncls).view(torch.int16).reshape(2, T, B, ted)
        assert torch.equal(none, without)
    # every sample kept: wd_emb_combine itself
    ones = torch.ones(B, dtype=torch.uint8, device=DEV)
    allk = keep_run(ones.data_ptr(), lview.data_ptr(), yd.data_ptr(), NCLS).view(torch.int16).reshape(2, T, B, ted)
    assert torch.equal(allk, with_label)
    G.assert_untouched(tbuf, tview, "time")
    G.assert_untouched(lbuf, lview, "label")
    # a keep mask without a table is refused
    pl = torch.zeros(2, B, ted, dtype=torch.bfloat16, device=DEV)
    assert lib.wd_emb_combine_keep(tview.data_ptr(), None, None, kd.data_ptr(), NCLS, 1, B, ted, pl[0].data_ptr(), pl[1].data_ptr(), ted,
                                   _st()) == N.WD_EINVAL
    torch.cuda.synchronize()
    assert not bool(pl.float().any())


@pytest.mark.parametrize("i64", [1, 0])
def test_embedding_bwd_skips_ids_outside_the_table(i64):
    """The contract ``label_emb:bwd`` relies on when it is handed ``y_eff``: a row with id -1 (or any id outside [0, vocab)) adds to
    no table row."""
    lib = N.lib()
    rows, vocab, c, ld = 9, 11, 40, 48
    g = torch.Generator().manual_seed(12)
    d = torch.randn(rows, ld, generator=g)
    ids = torch.tensor([3, -1, 3, vocab, 0, 10, -1, 3, vocab + 5])
    live = (ids >= 0) & (ids < vocab)
    assert 0 < int(live.sum()) < rows
    start = torch.randn(vocab, c, generator=g)
    idt = ids if i64 else ids.to(torch.int32)

    def run(id_t, d_t, acc):
        table = start.to(DEV) if acc else torch.full((vocab, c), float("nan"), device=DEV)
        idd, dd = id_t.to(DEV), d_t.contiguous().to(DEV)
        N.check(lib.wd_embedding_bwd(idd.data_ptr(), i64, id_t.numel(), dd.data_ptr(), ld, vocab, c, table.data_ptr(), acc, _st()),
                "wd_embedding_bwd")
        torch.cuda.synchronize()
        return table.cpu()

    for acc in (0, 1):
        masked, compact = run(idt, d, acc), run(idt[live], d[live], acc)
        assert bool(torch.isfinite(masked).all())
        assert torch.equal(masked.view(torch.int32), compact.view(torch.int32)), acc
    ref = torch.zeros(vocab, c, dtype=torch.float64).index_add_(0, ids[live], d[live, :c].double())
    assert float((run(idt, d, 0).double() - ref).abs().max()) < 1e-5
    assert not bool(run(idt, d, 0)[[1, 2, 4, 5, 6, 7, 8, 9]].any())  # writers no live row names: exactly zero
