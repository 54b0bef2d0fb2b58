"""Writer-style interpolation (``mix_rate``; unet.py:1558-1573, train.py:221-236), host side: the pair draws against the pairs the
reference's own models drew, and the oracle with the blended embedding against the reference's recorded forwards and
trajectories (``tests/golden/interp.npz``, written by ``tools/make_golden_interp.py`` from the reference's modules).

The oracle bars are those of ``tests/test_oracle_golden.py``: 2e-5 for a forward, 5e-5 for the states of a trajectory."""
import random

import torch
import torch.nn.functional as F

from oracle import ddpm_oracle as D
from oracle import unet_oracle as U
from tests._common import SMALL, load_golden, max_rel
from worddiffusion_amd import _native as N
from worddiffusion_amd.diffusion import STYLE_ID_MAX, draw_style_pairs
from worddiffusion_amd.synthetic import synthetic_tensor

CFG = dict(SMALL, num_classes=339)


class MixOracle(U.UNetOracle):
    """``UNetOracle`` with the label term of unet.py:1565-1573: one blended row for the whole batch, ``y`` unused."""
    pair = None
    mix_rate = None

    def embed(self, t, y):
        sd = self.sd
        e = U.timestep_embedding(t, self.cfg["model_channels"], dtype=self.dtype)
        e = F.linear(e, sd["time_embed.0.weight"], sd["time_embed.0.bias"])
        e = F.linear(F.silu(e), sd["time_embed.2.weight"], sd["time_embed.2.bias"])
        y1 = F.embedding(torch.tensor([self.pair[0]]), sd["label_emb.weight"])
        y2 = F.embedding(torch.tensor([self.pair[1]]), sd["label_emb.weight"])
        return e + ((1 - self.mix_rate) * y1 + self.mix_rate * y2)


def mix_oracle(variant, seed, dtype=torch.float32):
    sd = {k: torch.from_numpy(synthetic_tensor(k, s, seed)).to(dtype) for k, s in U.state_dict_shapes(CFG, variant)}
    orc = MixOracle(CFG, sd, variant, False)
    return orc


def reference_style_draws(n):
    """The draws of ``n`` reference forwards, written out (unet.py:1561-1564)."""
    out = []
    for _ in range(n):
        s1 = random.randint(0, 338)
        s2 = random.randint(0, 338)
        while s1 == s2:
            s2 = random.randint(0, 338)
        out.append((s1, s2))
    return out


def test_draw_style_pairs_are_the_pairs_the_reference_drew(golden_dir):
    g = load_golden(golden_dir, "interp")
    assert STYLE_ID_MAX == 338 and int(g["num_classes"]) == 339
    for tag, n in (("base", 1), ("phosc", 1)):
        random.seed(int(g[tag + "_rseed"]))
        assert draw_style_pairs(n) == [tuple(int(v) for v in g[tag + "_pair"])]
    for tag, n in (("cfg3", 14), ("cfg0", 7)):
        random.seed(int(g[tag + "_rseed"]))
        got = draw_style_pairs(n)
        assert g[tag + "_pairs"].shape == (n, 2)
        assert got == [tuple(int(v) for v in p) for p in g[tag + "_pairs"]]


def test_draw_style_pairs_leaves_random_in_the_reference_state():
    for k in (0, 7, 1003):
        for n in (1, 14, 999):
            random.seed(k)
            ref = reference_style_draws(n)
            state = random.getstate()
            random.seed(k)
            assert draw_style_pairs(n) == ref
            assert random.getstate() == state
    # a generator of the caller's own leaves the global one alone
    random.seed(5)
    state = random.getstate()
    rng = random.Random(5)
    mine = draw_style_pairs(3, rng=rng)
    assert random.getstate() == state
    assert mine == draw_style_pairs(3)
    assert all(a != b and 0 <= a <= 338 and 0 <= b <= 338 for a, b in mine)


def test_mix_oracle_reproduces_the_reference_forwards(golden_dir):
    g = load_golden(golden_dir, "interp")
    for tag, variant in (("base", "base"), ("phosc", "phosc")):
        orc = mix_oracle(variant, int(g[tag + "_seed"]))
        orc.pair, orc.mix_rate = [int(v) for v in g[tag + "_pair"]], float(g["mix_rate"])
        with torch.no_grad():
            out = orc(torch.from_numpy(g[tag + "_x"]), torch.from_numpy(g[tag + "_t"]), torch.from_numpy(g[tag + "_context"]),
                      torch.from_numpy(g[tag + "_y"]))
        err = max_rel(out, g[tag + "_out"])
        print(f"interp oracle forward {tag}: max_rel {err:.3e}")
        assert err < 2e-5, tag


def oracle_trajectory(g, tag, dtype=torch.float32):
    """The reference loop (train.py:221-236) on the oracle, replayed with the recorded start, noise and pairs.  Returns the
    x handed to the model per step, every single prediction in call order and the guided prediction per step."""
    T, s = int(g[tag + "_T"]), float(g[tag + "_cfg_scale"])
    n = g[tag + "_labels"].shape[0]
    orc = mix_oracle("phosc", int(g[tag + "_seed"]), dtype)
    orc.dtype = dtype
    orc.mix_rate = float(g["mix_rate"])
    ctx = torch.tensor([D.label_padding(str(g[tag + "_word"]))] * n, dtype=torch.int64)
    y = torch.from_numpy(g[tag + "_labels"])
    pairs = [[int(v) for v in p] for p in g[tag + "_pairs"]]
    noise = torch.from_numpy(g[tag + "_noise"]).to(dtype)
    preds, guided, rec = [], [], []

    def model(x, t):
        orc.pair = pairs[len(preds)]
        first = orc(x, t, ctx, y)
        preds.append(first)
        if s > 0:
            orc.pair = pairs[len(preds)]
            second = orc(x, t, ctx, y)
            preds.append(second)
            first = torch.lerp(second, first, s)
        guided.append(first)
        return first

    with torch.no_grad():
        x0 = D.sampling(model, noise[0], list(noise[1:]), T, rec)
    return torch.stack(rec), torch.stack(preds), torch.stack(guided), x0


def test_mix_oracle_reproduces_the_reference_trajectories(golden_dir):
    g = load_golden(golden_dir, "interp")
    for tag, nfwd in (("cfg3", 14), ("cfg0", 7)):
        xs, preds, _, x0 = oracle_trajectory(g, tag)
        assert preds.shape == tuple(g[tag + "_pred"].shape) and preds.shape[0] == nfwd
        ex, ep = max_rel(xs, g[tag + "_x_per_step"]), max(max_rel(p, q) for p, q in zip(preds, g[tag + "_pred"]))
        print(f"interp oracle trajectory {tag}: x max_rel {ex:.3e}, single predictions max_rel {ep:.3e}")
        assert ex < 5e-5 and ep < 2e-5, tag
        img = ((x0 / 0.18215) / 2 + 0.5).clamp(0, 1)
        assert float((img - torch.from_numpy(g[tag + "_image"])).abs().max()) < 2e-4


def test_interpolation_entry_points_are_declared_and_bound():
    names = ("wd_emb_combine_mix", "wd_label_mix", "wd_ddpm_step_cfg")
    assert set(names) <= set(N.header_symbols()) and set(names) <= set(N._SIGS)


def test_mix_rate_without_interpolation_is_not_an_interpolating_call():
    """``_mix_setup`` is where a sampler decides; it needs no device.  A model built without args.interpolation ignores
    mix_rate (unet.py:1558) and the global generator is not consumed."""
    import types
    from worddiffusion_amd import Diffusion
    diff = Diffusion(noise_steps=8)
    random.seed(3)
    state = random.getstate()
    assert diff._mix_setup(types.SimpleNamespace(interpolation=False), 3, 0.37, None, 3) is None
    assert random.getstate() == state
    # reference mode: 2 (T - 1) pairs in loop order with guidance, T - 1 without
    g_pairs = draw_style_pairs(14)
    random.seed(3)
    tab, m, s = diff._mix_setup(types.SimpleNamespace(interpolation=True), 3, 0.37, None, 3)
    assert tab.shape == (2, 8, 3, 2) and s == 3.0 and torch.equal(m, torch.full((3,), 0.37))
    for k, i in enumerate(reversed(range(1, 8))):
        for f in range(2):
            assert [tuple(r) for r in tab[f, i].tolist()] == [g_pairs[2 * k + f]] * 3
    random.seed(3)
    tab, _, _ = diff._mix_setup(types.SimpleNamespace(interpolation=True), 3, 0.37, None, 0)
    assert tab.shape == (1, 8, 3, 2) and tuple(tab[0, 7, 0].tolist()) == g_pairs[0] and tuple(tab[0, 1, 2].tolist()) == g_pairs[6]
    # fixed pairs: no draw, the same pair at every step, whatever args.interpolation says
    state = random.getstate()
    tab, m, _ = diff._mix_setup(types.SimpleNamespace(interpolation=False), 3, torch.linspace(0, 1, 3), (3, 7), 3)
    assert random.getstate() == state
    assert tab.shape == (1, 8, 3, 2) and (tab == torch.tensor([3, 7], dtype=torch.int32)).all()
    assert torch.equal(m, torch.linspace(0, 1, 3))


def test_mix_setup_draws_the_pairs_it_always_drew_and_a_refused_call_draws_none():
    """The pairs of an accepted call: ``draw_style_pairs`` over the sampler's model-calling steps in loop order, forward by
    forward within a step, and ``random`` left after exactly that many draws.  ``mix_rate`` / ``style_pairs`` are validated before
    the draw, so a refused call leaves ``random`` where it was."""
    import types

    import pytest
    from worddiffusion_amd import Diffusion
    diff, n = Diffusion(noise_steps=8), 3
    model = types.SimpleNamespace(interpolation=True)
    skipping = diff._ddpm(lambda i: i in (7, 5, 2))
    cases = ((None, list(reversed(range(1, 8))), 8), (skipping, [7, 5, 2], 8), (diff._ddim([7, 4, 1], 0.0), [0, 1, 2], 3),
             (diff._dpmpp([6, 3], 2), [0, 1], 2))
    for k, (sampler, rows, T) in enumerate(cases):
        for cfg_scale, nf in ((3, 2), (0, 1)):
            random.seed(k)
            drawn = draw_style_pairs(nf * len(rows))
            state = random.getstate()
            want = torch.zeros((nf, T, n, 2), dtype=torch.int32)
            for j, i in enumerate(rows):
                for f in range(nf):
                    want[f, i] = torch.tensor(drawn[nf * j + f], dtype=torch.int32)
            random.seed(k)
            tab, m, s = diff._mix_setup(model, n, 0.37, None, cfg_scale, **({} if sampler is None else dict(sampler=sampler)))
            assert torch.equal(tab, want) and tab.dtype == torch.int32 and s == float(cfg_scale)
            assert random.getstate() == state
    random.seed(5)
    state = random.getstate()
    for mix_rate, style_pairs in ((torch.zeros(2), None), (0.5, (1, 2, 3)), (None, (1, 2)), (torch.zeros(4), (1, 2))):
        with pytest.raises(ValueError):
            diff._mix_setup(model, n, mix_rate, style_pairs, 3)
        assert random.getstate() == state
