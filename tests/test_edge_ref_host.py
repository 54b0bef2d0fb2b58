"""tests/_edge_ref.py - the host specification tests/test_gpu_edge_guard.py holds the edge kernels to - against functions the
project already trusts: the oracle's timestep embedding, positional encoding, schedule, reverse step and noise_images,
``F.unfold``, ``permute`` and the EMA expression of tests/test_gpu_training.py.  Exact equality where the specification is fp32
ordered, the GPU test's own bounds where it is float64.  A wrong specification must not be able to hide a wrong kernel; neither
must a case table that no longer reaches the second pass of a grid-stride loop."""
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ddpm_oracle as D
from oracle import unet_oracle as U
from tests import _edge_ref as E
from tests import _philox_ref as P


def test_step_tables_are_the_oracle_schedule():
    beta, alpha, ah = D.schedule(1000)
    ca, cb, cs, sa, sb = E.step_tables(1000)
    assert torch.equal(ca, 1 / torch.sqrt(alpha)) and torch.equal(cb, (1 - alpha) / torch.sqrt(1 - ah))
    assert torch.equal(cs, torch.sqrt(beta)) and torch.equal(sa, torch.sqrt(ah)) and torch.equal(sb, torch.sqrt(1 - ah))


@pytest.mark.parametrize("t", [999, 500, 2, 1, 0])
def test_ddpm_update_is_the_oracle_reverse_step(t):
    beta, alpha, ah = D.schedule(1000)
    ca, cb, cs, _, _ = E.step_tables(1000)
    x, eps, z = (E.rand((3, 4, 5, 7), 20 + i) for i in range(3))
    ref = D.reverse_step(beta, alpha, ah, x, eps, t, z)
    assert torch.equal(E.ddpm_update(x, eps, ca, cb, cs, t, z), ref)
    if t <= 1:  # z is not read
        assert torch.equal(E.ddpm_update(x, eps, ca, cb, cs, t, None), ref)
        assert torch.equal(E.ddpm_update(x, eps, ca, cb, cs, t, torch.full_like(x, float("nan"))), ref)
    else:
        assert not torch.equal(E.ddpm_update(x, eps, ca, cb, cs, t, torch.zeros_like(x)), ref)


@pytest.mark.parametrize("scale", E.GUIDE_SCALES)
def test_guided_eps_is_both_forms_of_lerp(scale):
    """At these weights the product is exact: the two-rounding form the kernel evaluates and a fused one are the same value."""
    first, second = E.rand((3, 515), 30), E.rand((3, 515), 31)
    f, s = first.numpy(), second.numpy()
    d = (f - s).astype(np.float32)
    sc = np.float32(scale)
    if abs(scale) >= 0.5:
        oms = np.float32(1.0) - sc
        two = (f - (d * oms).astype(np.float32)).astype(np.float32)
        exact = f.astype(np.float64) - d.astype(np.float64) * float(oms)
    else:
        two = (s + (sc * d).astype(np.float32)).astype(np.float32)
        exact = s.astype(np.float64) + float(sc) * d.astype(np.float64)
    got = E.guided_eps(first, second, scale)
    assert torch.equal(got, torch.from_numpy(two))
    assert torch.equal(got, torch.from_numpy(exact.astype(np.float32)))  # one rounding of the exact sum: the fused form
    with pytest.raises(AssertionError):
        E.guided_eps(first, second, 0.3)


def test_noise_images_is_the_oracle():
    _, _, ah = D.schedule(1000)
    _, _, _, sa, sb = E.step_tables(1000)
    x, eps = E.rand((6, 3, 5, 7), 40), E.rand((6, 3, 5, 7), 41)
    t = torch.tensor([1, 5, 300, 999, 0, 640], dtype=torch.int64)
    ref = D.noise_images(ah, x, t, eps)
    assert torch.equal(E.noise_images(x.reshape(6, -1), eps.reshape(6, -1), t, sa, sb), ref.reshape(6, -1))


@pytest.mark.parametrize("beta", E.EMA_BETAS)
def test_ema_update_is_the_training_expression(beta):
    ema, p = E.rand((100003,), 50), E.rand((100003,), 51)
    assert torch.equal(E.ema_update(ema, p, beta), ema * beta + (1 - beta) * p)  # tests/test_gpu_training.py, train.py:146-170


def test_layout_changes_are_permute():
    x = E.rand((3, 4, 21), 60)
    tok = E.nchw_to_tokens(x)
    assert torch.equal(tok, x.permute(0, 2, 1).reshape(3 * 21, 4))
    assert torch.equal(E.tokens_to_nchw(tok, 3), x)


@pytest.mark.parametrize("B,cin,h,w,kpad", [(3, 4, 8, 32, 64), (2, 1, 1, 1, 32), (2, 3, 5, 7, 32), (1, 4, 1, 9, 96)])
def test_im2col_is_unfold(B, cin, h, w, kpad):
    x = E.rand((B, cin, h, w), 70)
    got = E.im2col3x3(x, kpad)
    unf = F.unfold(x, 3, padding=1).reshape(B, cin, 9, h * w).permute(0, 3, 2, 1).reshape(B * h * w, 9 * cin)  # [tap][ci]
    assert torch.equal(got[:, :9 * cin], unf) and not got[:, 9 * cin:].any()


def test_embed_tokens_is_index_plus_the_oracle_positional_encoding():
    table, pe = E.rand((53, 64), 80), U.positional_encoding(10, 64)
    ids = torch.randint(0, 53, (4, 10), generator=torch.Generator().manual_seed(81))
    assert torch.equal(E.embed_tokens(ids.reshape(-1), table, pe, 10), (table[ids] + pe[:10]).reshape(40, 64))
    assert torch.equal(E.embed_tokens(ids.reshape(-1).to(torch.int32), table, None, 10), table[ids].reshape(40, 64))
    bad = torch.tensor([-3, 53 + 7, 0, 52])
    assert torch.equal(E.embed_tokens(bad, table, None, 10), table[[0, 52, 0, 52]])
    assert torch.equal(E.embed_tokens(bad, table, pe, 3), table[[0, 52, 0, 52]] + pe[[0, 1, 2, 0]])


@pytest.mark.parametrize("dim", E.TEMB_DIMS)
def test_timestep_embedding_is_the_oracle(dim):
    t = torch.tensor(E.TEMB_T["table"], dtype=torch.int64)
    got = E.timestep_embedding(t, E.temb_freqs(dim))
    assert got.dtype == torch.float64 and tuple(got.shape) == (1000, dim)
    assert float((got - U.timestep_embedding(t, dim, dtype=torch.float64)).abs().max()) <= 1e-15
    assert float((got - U.timestep_embedding(t, dim).double()).abs().max()) < E.TEMB_BOUND


def test_emb_combine_is_silu_of_the_sum():
    T, B, ted, ncls = 5, 3, 64, 11
    time_, label = E.rand((T, ted), 90), E.rand((ncls, ted), 91)
    y = torch.tensor([4, 0, 10])
    ref = F.silu(time_.double()[:, None, :] + label.double()[y][None]).reshape(T * B, ted)
    assert E.within(E.emb_combine(time_, label, y, B), ref, E.PLANE_BOUND)[0]
    assert float((E.emb_combine(time_, label, y, B) - ref).abs().max()) < 1e-14
    bad = torch.tensor([-5, 10 ** 6, 3])
    assert torch.equal(E.emb_combine(time_, label, bad, B), E.emb_combine(time_, label, torch.tensor([0, ncls - 1, 3]), B))
    nolab = F.silu(time_.double())[:, None, :].expand(T, B, ted).reshape(T * B, ted)
    assert float((E.emb_combine(time_, None, None, B) - nolab).abs().max()) < 1e-14
    # the bound can tell: one bf16 rounding (a lost lo plane) is outside it
    assert not E.within(ref.float().to(torch.bfloat16).double(), ref, E.PLANE_BOUND)[0]


def test_advance_clamps_at_zero():
    assert [E.advance(t, d) for t, d in E.ADVANCE_STEPS] == [1, 0, 0, 633, 0]
    assert {1, 256, 257, 1000} <= set(E.ADVANCE_BATCH)


def test_draws_are_the_philox_reference_under_the_pinned_key():
    z, r = E.draws(3, 12, 77, 6, 500)
    for b in range(3):
        for e4 in range(3):
            zz, rr = P.normal4(77, 6 + b, 500, e4)
            assert np.array_equal(z[b, 4 * e4:4 * e4 + 4], zz) and np.array_equal(r[b, 4 * e4:4 * e4 + 4], rr)
    assert E.draws_within(z.astype(np.float32), (z, r)) <= 2.0 ** -24 / E.DRAW_TOL * 1.5  # an fp32 rounding is far inside
    assert E.draws_within(np.roll(z, 4, axis=1).astype(np.float32), (z, r)) > 1.0  # a draw of another element is outside


# ------------------------------------------------------------------------------------------------ the case tables
@pytest.mark.parametrize("kernel", sorted(E.CASES))
def test_every_kernel_has_a_case_past_the_grid_cap_and_one_inside_a_block(kernel):
    assert E.GRID_CAP_ITEMS == 2048 * 256
    big = [c for c in E.CASES[kernel] if E.is_big(kernel, c)]
    assert big, kernel
    for c in big:
        total, per = E.items(kernel, c)
        tail = total - E.GRID_CAP_ITEMS
        assert 0 < tail < E.GRID_CAP_ITEMS and tail % E.BLOCK != 0, (kernel, c, tail)
        if per:  # the second pass begins inside the last sample
            assert E.GRID_CAP_ITEMS // per == total // per - 1 and E.GRID_CAP_ITEMS % per != 0, (kernel, c)
    small = [c for c in E.CASES[kernel] if E.items(kernel, c)[0] < E.BLOCK]
    assert small and any(E.items(kernel, c)[0] > 1 for c in small), kernel
    assert len({E.case_id(c) for c in E.CASES[kernel]}) == len(E.CASES[kernel])


def test_the_largest_specification_runs_in_seconds():
    """The whole-array draws of the large wd_randn / wd_ddpm_step case (the slowest thing the GPU test asks of the host) and the
    updates on them: a couple of seconds, so the GPU test compares every element and needs no windows."""
    c = next(c for c in E.CASES["wd_ddpm_step"] if E.is_big("wd_ddpm_step", c))
    ca, cb, cs, sa, sb = E.step_tables(1000)
    x, eps = E.rand((c["batch"], c["n"]), 1), E.rand((c["batch"], c["n"]), 2)
    t0 = time.perf_counter()
    E.draws.cache_clear()
    z, r = E.draws(c["batch"], c["n"], 77, 6, 500)
    E.ddpm_update(x, eps, ca, cb, cs, 500, torch.from_numpy(z.astype(np.float32)))
    E.noise_images(x, eps, torch.tensor([1, 500, 999, 3, 7]), sa, sb)
    E.ema_update(x, eps, 0.995)
    dt = time.perf_counter() - t0
    print(f"largest case on the host: {dt:.2f} s")
    assert z.shape == (c["batch"], c["n"]) and dt < 10.0, dt
