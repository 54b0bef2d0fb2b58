"""The numpy specification of wd_row_slots / wd_adamw_rows (tests/_rowopt_ref.py) against what it specifies: torch.optim.AdamW on
the rows as a tensor of their own, the anchor's fixed point, and the slot rules.  No GPU."""
import numpy as np
import torch

from tests import _rowopt_ref as R


def test_spec_without_anchor_is_torch_adamw():
    """anchor=None: torch.optim.AdamW(foreach=False) on a CPU [R, c] tensor, after steps 1 and 3, under the bar of
    test_fused_adamw_at_chunk_edges: |got - want| <= 1e-6 |want| + 1e-7 max|want|."""
    g = torch.Generator().manual_seed(4)
    vocab, c, rows = 9, 256, (7, 2, 4)
    table = torch.randn(vocab, c, generator=g)
    p = torch.nn.Parameter(table[list(rows)].clone())
    ref = torch.optim.AdamW([p], lr=1e-3, weight_decay=0.01, foreach=False)
    tab, m, v = table.numpy().copy(), np.zeros((3, c), np.float32), np.zeros((3, c), np.float32)
    for step in (1, 2, 3):
        gr = torch.randn(3, c, generator=g) * (0.1 * step)
        p.grad = gr.clone()
        ref.step()
        tab, m, v, _ = R.adamw_rows(tab, rows, gr.numpy(), m, v, step, lr=1e-3, weight_decay=0.01)
        if step == 2:
            continue
        want = p.detach().numpy()
        got = tab[list(rows)]
        err = np.abs(got - want)
        print(f"step {step}: worst |got - want| {err.max():.3e}")
        assert np.all(err <= 1e-6 * np.abs(want) + 1e-7 * np.abs(want).max())
        st = ref.state[p]
        for got_s, want_s in ((m, st["exp_avg"].numpy()), (v, st["exp_avg_sq"].numpy())):
            assert np.all(np.abs(got_s - want_s) <= 1e-6 * np.abs(want_s) + 1e-7 * np.abs(want_s).max())
    others = [r for r in range(vocab) if r not in rows]
    assert np.array_equal(tab[others], table.numpy()[others])


def test_row_at_its_anchor_stays_put():
    g = torch.Generator().manual_seed(5)
    table = torch.randn(4, 64, generator=g).numpy()
    rows = (3, 0)
    anchor = table[list(rows)].copy()
    z = np.zeros((2, 64), np.float32)
    tab, m, v, ema = R.adamw_rows(table, rows, z, z, z, 1, lr=1e-2, weight_decay=0.5, anchor=anchor, ema_table=table, ema_mode=1)
    assert np.array_equal(tab.view(np.int32), table.view(np.int32))
    assert np.array_equal(ema.view(np.int32), table.view(np.int32))
    assert not m.any() and not v.any()
    # away from the anchor the decay pulls towards it, not towards zero
    far = anchor + np.float32(1.0)
    tab, *_ = R.adamw_rows(table, rows, z, z, z, 1, lr=1e-2, weight_decay=0.5, anchor=far)
    assert np.all(np.abs(tab[list(rows)] - far) < np.abs(table[list(rows)] - far))


def test_gscale_scales_the_gradient_before_anything_else():
    g = torch.Generator().manual_seed(6)
    table, gr = torch.randn(3, 8, generator=g).numpy(), torch.randn(1, 8, generator=g).numpy()
    z = np.zeros((1, 8), np.float32)
    a = R.adamw_rows(table, (1,), gr, z, z, 1, gscale=0.25)
    b = R.adamw_rows(table, (1,), gr * np.float32(0.25), z, z, 1)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)


def test_ema_modes():
    g = torch.Generator().manual_seed(7)
    table, ema0, gr = (torch.randn(3, 8, generator=g).numpy() for _ in range(3))
    z = np.zeros((1, 8), np.float32)
    tab, _, _, e0 = R.adamw_rows(table, (2,), gr[:1], z, z, 1, ema_table=ema0, ema_mode=0)
    assert np.array_equal(e0, ema0)
    _, _, _, e1 = R.adamw_rows(table, (2,), gr[:1], z, z, 1, ema_table=ema0, ema_mode=1)
    assert np.array_equal(e1[2], tab[2]) and np.array_equal(e1[:2], ema0[:2])
    _, _, _, e2 = R.adamw_rows(table, (2,), gr[:1], z, z, 1, ema_table=ema0, ema_mode=2, ema_beta=0.9)
    want = ema0[2] * np.float32(0.9) + np.float32(1.0 - 0.9) * tab[2]
    assert np.array_equal(e2[2], want) and np.array_equal(e2[:2], ema0[:2])


def test_slots_cover_absent_ids_ids_outside_the_table_and_minus_one():
    rows = (9, 4, 6)
    ids = np.array([4, 9, 5, -1, 6, 10 ** 12, -7, 4], dtype=np.int64)
    assert R.row_slots(ids, rows).tolist() == [1, 0, -1, -1, 2, -1, -1, 1]
    d = np.arange(8 * 4, dtype=np.float32).reshape(8, 4)
    out = R.embedding_bwd(R.row_slots(ids, rows), d, 3)
    assert np.array_equal(out[0], d[1]) and np.array_equal(out[1], d[0] + d[7]) and np.array_equal(out[2], d[4])
