"""wd_row_slots and wd_adamw_rows on windows of NaN-filled buffers (tests/_guard.py), bit for bit against their numpy specification
(tests/_rowopt_ref.py): pitched tables, an EMA table of another pitch, the three EMA modes, with and without anchor and gradient
scale; unlisted rows and every guard band untouched in both tables; the anchor-free form against wd_adamw_multi; the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _guard as G  # noqa: E402
from tests import _rowopt_ref as R  # noqa: E402
from worddiffusion_amd import _native as N  # noqa: E402

DEV = "cuda:0"
RMAX = N.DEFINES["WD_ROWS_MAX"]
HYPER = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.05)


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def crows(rows):
    return (C.c_int * len(rows))(*rows)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def adamw_rows(table, ld, c, rows, vocab, grad, m, v, anchor, ema, ema_ld, step, ema_mode, ema_beta, gscale):
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    return N.lib().wd_adamw_rows(ptr(table), ld, c, crows(rows), len(rows), vocab, ptr(grad), ptr(m), ptr(v), ptr(anchor), ptr(ema),
                                 ema_ld, HYPER["lr"], HYPER["beta1"], HYPER["beta2"], HYPER["eps"], HYPER["weight_decay"], step,
                                 ema_mode, ema_beta, ptr(gscale), stream())


# ------------------------------------------------------------------------------------------------------------- slots
@pytest.mark.parametrize("nrows", [1, 3, RMAX])
def test_row_slots_matches_the_specification(nrows):
    vocab, n = 200, 301  # more than one workgroup of ids
    g = np.random.RandomState(nrows)
    rows = [int(r) for r in g.permutation(vocab)[:nrows]]
    ids = g.randint(0, vocab, size=n).astype(np.int64)
    ids[:6] = [-1, vocab, 1 << 40, -(1 << 40), rows[0], rows[-1]]
    ids_buf, ids_v = G.guarded_flat(n, torch.float64, device=DEV)  # (int64 ids behind a poisoned frame of the same width)
    ids_v.view(torch.int64).copy_(torch.from_numpy(ids))
    out_buf, out_v = G.guarded_flat(n, torch.float64, device=DEV)
    rc = N.lib().wd_row_slots(ids_v.data_ptr(), n, crows(rows), nrows, vocab, out_v.data_ptr(), stream())
    torch.cuda.synchronize()
    assert rc == N.WD_OK
    want = R.row_slots(ids, rows)
    assert np.array_equal(out_v.view(torch.int64).cpu().numpy(), want)
    assert (want >= 0).sum() >= 2 and (want < 0).sum() >= 4
    G.assert_untouched(out_buf, out_v, "slots")
    G.assert_untouched(ids_buf, ids_v, "ids")


def test_slots_feed_the_compact_embedding_backward():
    """slots are wd_embedding_bwd's ids with vocab = nrows: the compact gradient equals the listed rows of the full table's."""
    lib, vocab, c, n, rows = N.lib(), 11, 256, 7, [9, 4, 6]
    g = torch.Generator().manual_seed(3)
    ids = torch.tensor([4, 9, 5, 4, 0, 6, 4], dtype=torch.int64, device=DEV)
    d = torch.randn(n, c, generator=g).to(DEV)
    full = torch.empty(vocab, c, device=DEV)
    slots = torch.empty(n, dtype=torch.int64, device=DEV)
    buf, compact = G.guarded(len(rows), c, c, 0, torch.float32, device=DEV)
    assert lib.wd_embedding_bwd(ids.data_ptr(), 1, n, d.data_ptr(), c, vocab, c, full.data_ptr(), 0, stream()) == N.WD_OK
    assert lib.wd_row_slots(ids.data_ptr(), n, crows(rows), len(rows), vocab, slots.data_ptr(), stream()) == N.WD_OK
    assert lib.wd_embedding_bwd(slots.data_ptr(), 1, n, d.data_ptr(), c, len(rows), c, compact.data_ptr(), 0, stream()) == N.WD_OK
    torch.cuda.synchronize()
    assert torch.equal(bits(compact), bits(full[rows]))
    assert np.array_equal(compact.cpu().numpy(), R.embedding_bwd(R.row_slots(ids.cpu().numpy(), rows), d.cpu().numpy(), len(rows)))
    G.assert_untouched(buf, compact, "compact gradient")


# ------------------------------------------------------------------------------------------------------------- AdamW
FORMS = [(0, False, False), (1, True, False), (2, False, True), (2, True, True)]  # (ema_mode, anchor, gscale)


@pytest.mark.parametrize("ema_mode,anchored,scaled", FORMS, ids=["plain", "ema1+anchor", "ema2+gscale", "ema2+anchor+gscale"])
@pytest.mark.parametrize("nrows", [1, 3, RMAX])
@pytest.mark.parametrize("c", [256, 1280])
def test_adamw_rows_matches_the_specification(c, nrows, ema_mode, anchored, scaled):
    vocab, ld, col0, ema_ld, ema_col0 = nrows + 5, c + 24, 8, c + 64, 32
    g = torch.Generator().manual_seed(c + 7 * nrows + ema_mode)
    rows = [int(r) for r in torch.randperm(vocab, generator=g)[:nrows]]
    rnd = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    table0, ema0 = rnd(vocab, c), rnd(vocab, c)
    tbuf, table = G.pitched(table0, ld, col0, device=DEV)
    ebuf, ema = G.pitched(ema0, ema_ld, ema_col0, device=DEV)
    compact = {}
    for name, val in (("grad", rnd(nrows, c) * 0.1), ("m", rnd(nrows, c) * 0.05), ("v", rnd(nrows, c).square() * 0.01),
                      ("anchor", rnd(nrows, c))):
        buf, view = G.guarded_flat(nrows * c, torch.float32, device=DEV)
        view.copy_(val.reshape(-1))
        compact[name] = (buf, view, val)
    gs = torch.tensor([0.0, 0.37], device=DEV)
    step, ema_beta = 3, 0.9
    rc = adamw_rows(table, ld, c, rows, vocab, compact["grad"][1], compact["m"][1], compact["v"][1],
                    compact["anchor"][1] if anchored else None, ema if ema_mode else None, ema_ld, step, ema_mode, ema_beta,
                    gs[1:] if scaled else None)
    torch.cuda.synchronize()
    assert rc == N.WD_OK
    want_t, want_m, want_v, want_e = R.adamw_rows(
        table0.numpy(), rows, compact["grad"][2].numpy(), compact["m"][2].numpy(), compact["v"][2].numpy(), step,
        anchor=compact["anchor"][2].numpy() if anchored else None, ema_table=ema0.numpy() if ema_mode else None, ema_mode=ema_mode,
        ema_beta=ema_beta, gscale=np.float32(0.37) if scaled else None, **HYPER)
    for name, got, want in (("table", table, want_t), ("exp_avg", compact["m"][1], want_m.reshape(-1)),
                            ("exp_avg_sq", compact["v"][1], want_v.reshape(-1)),
                            ("ema", ema, want_e if ema_mode else ema0.numpy())):
        assert torch.equal(bits(got), bits(torch.from_numpy(np.ascontiguousarray(want)))), name
    # unlisted rows, in both tables, and every guard band
    others = [r for r in range(vocab) if r not in rows]
    assert torch.equal(bits(table[others]), bits(table0[others])) and torch.equal(bits(ema[others]), bits(ema0[others]))
    assert not torch.equal(bits(table[rows]), bits(table0[rows]))
    G.assert_untouched(tbuf, table, "table")
    G.assert_untouched(ebuf, ema, "ema table")
    for name in ("grad", "anchor"):
        assert torch.equal(bits(compact[name][1]), bits(compact[name][2].reshape(-1))), name + " was written"
    for name, (buf, view, _) in compact.items():
        G.assert_untouched(buf, view, name)


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "gscale"])
def test_one_row_without_anchor_is_wd_adamw_multi(scaled):
    """anchor=None: one row updated by wd_adamw_rows equals the same data updated by wd_adamw_multi as a tensor of its own."""
    lib, c, vocab, row = N.lib(), 1280, 5, 3
    g = torch.Generator().manual_seed(11)
    table0, ema0 = torch.randn(vocab, c, generator=g), torch.randn(vocab, c, generator=g)
    grad, m0, v0 = torch.randn(1, c, generator=g) * 0.1, torch.randn(1, c, generator=g) * 0.05, torch.rand(1, c, generator=g) * 0.01
    gs = torch.tensor([0.61], device=DEV)
    got = [t.clone().to(DEV) for t in (table0, m0, v0, ema0)]
    ref = [t.clone().to(DEV) for t in (table0[row], m0[0], v0[0], ema0[row])]
    gd = grad.to(DEV)
    rec = N.WdAdamwTableEntry(ref[0].data_ptr(), gd.data_ptr(), ref[1].data_ptr(), ref[2].data_ptr(), ref[3].data_ptr(), c, 0)
    tab = torch.frombuffer((N.WdAdamwTableEntry * 1)(rec), dtype=torch.uint8).to(DEV)
    hyper = (HYPER["lr"], HYPER["beta1"], HYPER["beta2"], HYPER["eps"], HYPER["weight_decay"])
    for step in (1, 2):
        assert adamw_rows(got[0], c, c, [row], vocab, gd, got[1], got[2], None, got[3], c, step, 2, 0.995,
                          gs if scaled else None) == N.WD_OK
        if scaled:
            assert lib.wd_adamw_multi_scaled(tab.data_ptr(), 1, 1, *hyper, step, 2, 0.995, gs.data_ptr(), stream()) == N.WD_OK
        else:
            assert lib.wd_adamw_multi(tab.data_ptr(), 1, 1, *hyper, step, 2, 0.995, stream()) == N.WD_OK
    torch.cuda.synchronize()
    for name, a, b in (("p", got[0][row], ref[0]), ("m", got[1][0], ref[1]), ("v", got[2][0], ref[2]), ("ema", got[3][row], ref[3])):
        assert torch.equal(bits(a), bits(b)), name
    assert not torch.equal(got[0][row].cpu(), table0[row])


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing():
    lib, c, vocab, n = N.lib(), 256, 8, 5
    bufs = {k: torch.full((vocab, c), 2.0, device=DEV) for k in ("table", "ema", "grad", "m", "v", "anchor")}
    ids = torch.zeros(n, dtype=torch.int64, device=DEV)
    slots = torch.full((n,), 77, dtype=torch.int64, device=DEV)
    gs = torch.ones(2, device=DEV)
    good = dict(table=bufs["table"], ld=c, c=c, rows=[1, 2], vocab=vocab, grad=bufs["grad"], m=bufs["m"], v=bufs["v"],
                anchor=bufs["anchor"], ema=bufs["ema"], ema_ld=c, step=1, ema_mode=2, ema_beta=0.9, gscale=gs)
    off = lambda t: t.reshape(-1)[1:]  # noqa: E731  (4 bytes past a 16-byte boundary)
    bad = [("nrows 0", dict(rows=[])), ("nrows > WD_ROWS_MAX", dict(rows=list(range(RMAX + 1)), vocab=RMAX + 1)),
           ("row < 0", dict(rows=[1, -1])), ("row >= vocab", dict(rows=[vocab])), ("duplicate rows", dict(rows=[3, 1, 3])),
           ("c % 4", dict(c=254)), ("ld % 4", dict(ld=c + 2)), ("ema_ld % 4", dict(ema_ld=c + 2)), ("ld < c", dict(ld=c - 4)),
           ("NULL table", dict(table=None)), ("NULL grad", dict(grad=None)), ("NULL m", dict(m=None)), ("NULL v", dict(v=None)),
           ("table alignment", dict(table=off(bufs["table"]))), ("grad alignment", dict(grad=off(bufs["grad"]))),
           ("m alignment", dict(m=off(bufs["m"]))), ("v alignment", dict(v=off(bufs["v"]))),
           ("anchor alignment", dict(anchor=off(bufs["anchor"]))), ("ema alignment", dict(ema=off(bufs["ema"]))),
           ("step 0", dict(step=0)), ("ema_mode 3", dict(ema_mode=3))]
    for what, change in bad:
        assert adamw_rows(**dict(good, **change)) == N.WD_EINVAL, what
    null_rows = lib.wd_adamw_rows(bufs["table"].data_ptr(), c, c, None, 2, vocab, bufs["grad"].data_ptr(), bufs["m"].data_ptr(),
                                  bufs["v"].data_ptr(), None, None, 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0, 0.9, None, stream())
    assert null_rows == N.WD_EINVAL
    sl = lambda ids_, n_, rows_, nrows_, vocab_, out_: lib.wd_row_slots(ids_, n_, rows_, nrows_, vocab_, out_, stream())  # noqa: E731
    ip, sp = ids.data_ptr(), slots.data_ptr()
    for what, rc in (("NULL ids", sl(None, n, crows([1]), 1, vocab, sp)), ("NULL rows", sl(ip, n, None, 1, vocab, sp)),
                     ("NULL slots", sl(ip, n, crows([1]), 1, vocab, None)), ("n 0", sl(ip, 0, crows([1]), 1, vocab, sp)),
                     ("nrows 0", sl(ip, n, crows([1]), 0, vocab, sp)),
                     ("nrows > WD_ROWS_MAX", sl(ip, n, crows(list(range(RMAX + 1))), RMAX + 1, RMAX + 1, sp)),
                     ("row < 0", sl(ip, n, crows([-1]), 1, vocab, sp)), ("row >= vocab", sl(ip, n, crows([vocab]), 1, vocab, sp)),
                     ("duplicate rows", sl(ip, n, crows([2, 2]), 2, vocab, sp))):
        assert rc == N.WD_EINVAL, what
    torch.cuda.synchronize()
    assert all(bool((t == 2.0).all()) for t in bufs.values()) and bool((slots == 77).all())
    assert adamw_rows(**good) == N.WD_OK and sl(ip, n, crows([1]), 1, vocab, sp) == N.WD_OK  # the unchanged call is accepted
    torch.cuda.synchronize()
